// smallconv_train.hip -- conv2d(c -> c) + batch_normalization(training=True) + LeakyReLU of the TRAINING step on [N*K]-row tensors, fused.
//
//   LFA mlp2 of building_block (PointSegment/RandLANet.py:331; helper_tf_util.conv2d :115-170): z = lrelu(BN(x . W + b)), x = f_xyz rows,
//   c = d_out / 2 = 8 / 32 / 64 at encoder levels 0-2 of a batch of 8 x 180 000 points: 23 M / 5.8 M / 1.4 M rows.
//
// Op by op the pre-BatchNorm product y is written, read for the statistics, read again and written normalised; and in the backward
// BatchNorm's two passes read (dz, y) each, write dy, which the weight-gradient GEMM and the input-gradient GEMM read again: 14 passes
// over [rows, c] tensors.  Here y is never stored: a 16-row tile of x goes to LDS and y is recomputed from it on the fp32 MFMA wherever it
// is needed (c^2 MACs per row: nothing against the memory passes).
//   forward   sums  : per-channel sum y, sum y^2 (fp64 accumulators: the variance is a difference of nearly equal sums), sum x
//             apply : z = lrelu((y - mean) gamma invstd + beta) -> rows
//   backward  sums  : with xh = (y - mean) invstd, g = dz lrelu'(.):  S1 = sum g, S2 = sum g xh, XS = sum xh, A = x^T g, G = x^T xh
//                     (the two c x c products on the MFMA with the 16 rows of a tile as K, accumulated in registers per wave)
//             apply : dy = gamma invstd (g - S1/M - xh S2/M);  dx = dy . W^T -> rows (or added to an existing gradient)
//   and the caller finishes  dW = gamma invstd (A - (sum x) x S1/M - G . S2/M),  db, dgamma = S2, dbeta = S1  on the [c, c] sums
//   (train.py; under SyncBN that is also where the sums of all ranks meet).
// 8 passes instead of 14.  Sums are per-workgroup partials merged in a fixed order (deterministic).  c in {8, 16, 32, 64}.
// The tile mechanics (geometry, the tile's way global -> registers -> LDS and back, weight staging, the two MFMA loops, the workgroup tail)
// are convbn_tile.h's, shared with rectconv_train.hip.  This file's own: bfloat16 rows (XB), the unaligned fallback (a.vec == 0: 4-byte
// accesses in the accumulator layout), the FULL sums and sum x.
#include "convbn_tile.h"
#include "reduce_partials.h"

namespace ps {

struct ScArgs {
    const float* x;      // [R, C] rows (ldx)
    const float* w;      // [C, C] row-major
    const float* b;      // [C]
    const float* mean; const float* invstd; const float* scale; const float* beta;  // [C]; scale = gamma invstd
    const float* m1; const float* m2;  // [C] S1 / M, S2 / M (backward apply)
    float mscale;        // m1 / m2 hold the raw sums S1 / S2 of all ranks: multiplied by this (1 / rows of all ranks); 1 when they are means
    const float* dz;     // [R, C] (lddz)
    float* out;          // apply: z rows (ldo);  backward apply: dx rows (ldo)
    void* part;          // per-workgroup partial sums
    int64_t R;
    int ldx, lddz, ldo, accum;
    int vec;             // dz / out rows are 16-byte aligned with pitches % 4 == 0: tiles travel as float4 through LDS
    int x_bf16;          // x rows (and apply's out rows) are STORED as bfloat16 (ps_set_train_act_bf16): ldx / ldo in elements
    int bf16;            // bf16-MLP mode: the operands of the three products (x and w; dy and w^T; x and dy) are rounded to bfloat16 (RNE) first and
                         // multiplied on the fp32 MFMA (exact products, fp32 accumulation: the values of a bf16 MFMA with fp32 accumulate)
};

// the square case of convbn_tile.h: one padded width G::COP, one weight pitch G::PWO (= PWI), one tile pitch G::PX (= PZ)
template <int C>
using ScGeom = ConvGeom<C, C>;
template <int C>
using ScTile = RowTile<C, ScGeom<C>::PX>;

constexpr int kScWaves = 4;

// ---- forward: statistics (sum y, sum y^2 in fp64; sum x in fp32) ---------------------------------------------------------------
// partial layout per workgroup (doubles): sy[CP] | sq[CP] | sx[CP]
template <int C, bool XB>  // XB: x rows (and apply's output rows) are stored as bfloat16 -- a compile-time switch: a run-time branch around the
                           // tile loads made the compiler drain every load in flight at the join (bwd apply 0.66 -> 0.80 ms)
__global__ __launch_bounds__(kScWaves * 64) void sc_sums_kernel(ScArgs a)
{
    using G = ScGeom<C>;
    constexpr int NT = G::NTO;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* W = smem;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, g = lane >> 4, c16 = lane & 15;
    float* A = smem + G::COP * G::PWO + wave * 16 * G::PX;
    double* red = reinterpret_cast<double*>(smem + G::COP * G::PWO + kScWaves * 16 * G::PX);  // [kScWaves][3 CP]
    stage_w<C, C, kScWaves * 64>(a.w, W, nullptr, a.bf16 != 0);
    __syncthreads();
    const Cols<NT> bias(a.b, c16, C);
    double sy[NT], sq[NT], sx[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) { sy[t] = 0.; sq[t] = 0.; sx[t] = 0.; }
    const int64_t tiles = (a.R + 15) / 16, tstride = (int64_t)gridDim.x * kScWaves;
    int64_t tl = (int64_t)blockIdx.x * kScWaves + wave;
    ScTile<C> xr;
    if (tl < tiles) xr.template fetch_any<XB>(a.x, a.ldx, tl * 16, a.R, lane);
    for (; tl < tiles; tl += tstride) {
        const int64_t r0 = tl * 16;
        xr.template expand<XB>(), xr.commit(A, lane, a.bf16 != 0);
        wave_lds_sync();
        if (tl + tstride < tiles) xr.template fetch_any<XB>(a.x, a.ldx, (tl + tstride) * 16, a.R, lane);
#pragma unroll
        for (int ct = 0; ct < NT; ++ct) {
            const f32x4 y = tile_product<G::CIP, G::PX, G::PWO>(A, W, ct, lane);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (r0 + 4 * g + r < a.R) {
                    const double yd = (double)(y[r] + bias.v[ct]);
                    sy[ct] += yd;
                    sq[ct] = __builtin_fma(yd, yd, sq[ct]);
                    sx[ct] += (double)A[(4 * g + r) * G::PX + ct * 16 + c16];
                }
            }
        }
        wave_lds_sync();
    }
    cols_to_lds(red + wave * 3 * G::COP, G::COP, lane, sy, sq, sx);
    wg_merge<double, kScWaves>(red, 3 * G::COP, static_cast<double*>(a.part) + (size_t)blockIdx.x * 3 * G::COP);
}

// ---- forward: normalise + LeakyReLU -> rows --------------------------------------------------------------------------------------
template <int C, bool XB>
__global__ __launch_bounds__(kScWaves * 64) void sc_apply_kernel(ScArgs a)
{
    using G = ScGeom<C>;
    constexpr int NT = G::NTO;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* W = smem;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, g = lane >> 4, c16 = lane & 15;
    float* A = smem + G::COP * G::PWO + wave * 16 * G::PX;
    stage_w<C, C, kScWaves * 64>(a.w, W, nullptr, a.bf16 != 0);
    __syncthreads();
    const Cols<NT> bias(a.b, c16, C), mu(a.mean, c16, C), sc(a.scale, c16, C), be(a.beta, c16, C);
    const int64_t tiles = (a.R + 15) / 16, tstride = (int64_t)gridDim.x * kScWaves;
    int64_t tl = (int64_t)blockIdx.x * kScWaves + wave;
    ScTile<C> xr;
    if (tl < tiles) {
        xr.template fetch_any<XB>(a.x, a.ldx, tl * 16, a.R, lane);
        xr.template expand<XB>(), xr.commit(A, lane, a.bf16 != 0);
    }
    wave_lds_sync();
    for (; tl < tiles; tl += tstride) {
        const int64_t r0 = tl * 16;
        const bool more = tl + tstride < tiles;
        if (more) xr.template fetch_any<XB>(a.x, a.ldx, (tl + tstride) * 16, a.R, lane);
        f32x4 z[NT];
#pragma unroll
        for (int ct = 0; ct < NT; ++ct) {
            const f32x4 y = tile_product<G::CIP, G::PX, G::PWO>(A, W, ct, lane);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float t = __builtin_fmaf((y[r] + bias.v[ct]) - mu.v[ct], sc.v[ct], be.v[ct]);
                z[ct][r] = t < 0.f ? 0.2f * t : t;
            }
        }
        if (a.vec) {  // z staged in the (now dead) x tile, 16-byte stores
            wave_lds_sync();
#pragma unroll
            for (int ct = 0; ct < NT; ++ct)
#pragma unroll
                for (int r = 0; r < 4; ++r) A[(4 * g + r) * G::PX + ct * 16 + c16] = z[ct][r];
            wave_lds_sync();
            ScTile<C> o;
            o.take(A, lane);
            wave_lds_sync();
            if (more) xr.template expand<XB>(), xr.commit(A, lane, a.bf16 != 0);
            o.template put_any<XB>(a.out, a.ldo, r0, a.R, lane);
        } else {
#pragma unroll
            for (int ct = 0; ct < NT; ++ct) {
                const int col = ct * 16 + c16;
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (col < C && r0 + 4 * g + r < a.R) a.out[(size_t)(r0 + 4 * g + r) * a.ldo + col] = z[ct][r];
            }
            wave_lds_sync();
            if (more) xr.template expand<XB>(), xr.commit(A, lane, a.bf16 != 0);
        }
        wave_lds_sync();
    }
}

// ---- backward: sums --------------------------------------------------------------------------------------------------------------
// partial layout per workgroup (floats): S1[CP] | S2[CP] | XS[CP] | A[CP][CP] | G[CP][CP]
// FULL = false: only S1 | S2 | XS (the weight gradient then comes out of sc_bwd_apply_kernel<C, true, XB> as x^T dy)
template <int C, bool FULL, bool XB>
__global__ __launch_bounds__(kScWaves * 64) void sc_bwd_sums_kernel(ScArgs a)
{
    using G = ScGeom<C>;
    constexpr int NT = G::NTO, CP = G::COP, NV = FULL ? 3 * CP + 2 * CP * CP : 3 * CP;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* W = smem;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, g = lane >> 4, c16 = lane & 15;
    float* A = smem + CP * G::PWO + wave * 3 * 16 * G::PX;  // x tile | g tile | xh tile
    float* T1 = A + 16 * G::PX;
    float* T2 = T1 + 16 * G::PX;
    stage_w<C, C, kScWaves * 64>(a.w, W, nullptr, a.bf16 != 0);
    __syncthreads();
    const Cols<NT> bias(a.b, c16, C), mu(a.mean, c16, C), is(a.invstd, c16, C), sc(a.scale, c16, C), be(a.beta, c16, C);
    float s1[NT] = {}, s2[NT] = {}, xs[NT] = {};
    f32x4 aw[NT][NT] = {}, gw[NT][NT] = {};
    // vec: the dz tile travels like the x tile (16-byte loads one tile ahead, through LDS tile T1) instead of as 4-byte loads in the
    // accumulator layout
    const int64_t tiles = (a.R + 15) / 16, tstride = (int64_t)gridDim.x * kScWaves;
    int64_t tl = (int64_t)blockIdx.x * kScWaves + wave;
    ScTile<C> xr, zr;
    if (tl < tiles) {
        xr.template fetch_any<XB>(a.x, a.ldx, tl * 16, a.R, lane);
        if (a.vec) zr.template fetch_any<XB>(a.dz, a.lddz, tl * 16, a.R, lane);  // (gradient rows in the format of the activation rows)
    }
    for (; tl < tiles; tl += tstride) {
        const int64_t r0 = tl * 16;
        xr.template expand<XB>(), xr.commit(A, lane, a.bf16 != 0);
        if (a.vec) zr.template expand<XB>(), zr.commit(T1, lane);
        wave_lds_sync();
        if (tl + tstride < tiles) {
            xr.template fetch_any<XB>(a.x, a.ldx, (tl + tstride) * 16, a.R, lane);
            if (a.vec) zr.template fetch_any<XB>(a.dz, a.lddz, (tl + tstride) * 16, a.R, lane);
        }
#pragma unroll
        for (int ct = 0; ct < NT; ++ct) {
            const f32x4 y = tile_product<G::CIP, G::PX, G::PWO>(A, W, ct, lane);
            const int col = ct * 16 + c16;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool live = col < C && r0 + 4 * g + r < a.R;
                const float yc = (y[r] + bias.v[ct]) - mu.v[ct];
                const float xh = live ? yc * is.v[ct] : 0.f;
                float gv = !live ? 0.f : a.vec ? T1[(4 * g + r) * G::PX + col] : a.dz[(size_t)(r0 + 4 * g + r) * a.lddz + col];
                if (__builtin_fmaf(yc, sc.v[ct], be.v[ct]) <= 0.f) gv *= 0.2f;
                s1[ct] += gv;
                s2[ct] = __builtin_fmaf(gv, xh, s2[ct]);
                xs[ct] += xh;
                if (FULL) {
                    T1[(4 * g + r) * G::PX + col] = gv;
                    T2[(4 * g + r) * G::PX + col] = xh;
                }
            }
        }
        wave_lds_sync();
        if (FULL) xt_mma<NT, NT, G::PX, G::PX, true>(A, T1, T2, aw, gw, lane);  // A += x^T g, G += x^T xh
        wave_lds_sync();
    }
    // the workgroup's partial: waves add up through LDS in order (weights and tiles are dead: the buffer is sized for kScWaves x NV)
    __syncthreads();
    float* red = smem;
    float* r = red + (size_t)wave * NV;
    cols_to_lds(r, CP, lane, s1, s2, xs);
    if (FULL) acc_to_lds(aw, r + 3 * CP, CP, lane), acc_to_lds(gw, r + 3 * CP + CP * CP, CP, lane);
    wg_merge<float, kScWaves>(red, NV, static_cast<float*>(a.part) + (size_t)blockIdx.x * NV);
}

// ---- backward: input gradient ----------------------------------------------------------------------------------------------------
// WG = true: also the weight / bias gradient dW = x^T dy, db = sum dy as per-workgroup partials (dW[CP][CP] | db[CP]) in a.part
template <int C, bool WG, bool XB>
__global__ __launch_bounds__(kScWaves * 64) void sc_bwd_apply_kernel(ScArgs a)
{
    using G = ScGeom<C>;
    constexpr int NT = G::NTO, CP = G::COP;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* W = smem;
    float* WT = smem + CP * G::PWO;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, g = lane >> 4, c16 = lane & 15;
    float* A = smem + 2 * CP * G::PWO + wave * 2 * 16 * G::PX;  // x tile | dy tile
    float* T1 = A + 16 * G::PX;
    stage_w<C, C, kScWaves * 64>(a.w, W, WT, a.bf16 != 0);
    __syncthreads();
    const Cols<NT> bias(a.b, c16, C), mu(a.mean, c16, C), is(a.invstd, c16, C), sc(a.scale, c16, C), be(a.beta, c16, C);
    const Cols<NT> m1(a.m1, c16, C, a.mscale), m2(a.m2, c16, C, a.mscale);
    f32x4 dw[NT][NT] = {};
    float dbs[NT] = {};
    // vec: x, dz and (accumulate) the old dx rows of the NEXT tile are requested before this tile's work starts; the dz tile sits in T1 and is
    // replaced in place by dy; dx is staged in the x tile once the weight-gradient product has read it, and leaves as 16-byte stores
    const int64_t tiles = (a.R + 15) / 16, tstride = (int64_t)gridDim.x * kScWaves;
    int64_t tl = (int64_t)blockIdx.x * kScWaves + wave;
    const bool vec = a.vec != 0, acc_old = vec && a.accum;
    ScTile<C> xr, zr, old_next;
    if (tl < tiles) {
        xr.template fetch_any<XB>(a.x, a.ldx, tl * 16, a.R, lane);
        if (vec) zr.template fetch_any<XB>(a.dz, a.lddz, tl * 16, a.R, lane);  // (gradient rows dz / dx: the format of the activation rows)
        if (acc_old) old_next.template fetch_any<XB>(a.out, a.ldo, tl * 16, a.R, lane);
        xr.template expand<XB>(), xr.commit(A, lane, a.bf16 != 0);
        if (vec) zr.template expand<XB>(), zr.commit(T1, lane);
    }
    wave_lds_sync();
    for (; tl < tiles; tl += tstride) {
        const int64_t r0 = tl * 16;
        const bool more = tl + tstride < tiles;
        ScTile<C> old_cur = old_next;
        if (more) {
            xr.template fetch_any<XB>(a.x, a.ldx, (tl + tstride) * 16, a.R, lane);
            if (vec) zr.template fetch_any<XB>(a.dz, a.lddz, (tl + tstride) * 16, a.R, lane);
            if (acc_old) old_next.template fetch_any<XB>(a.out, a.ldo, (tl + tstride) * 16, a.R, lane);
        }
#pragma unroll
        for (int ct = 0; ct < NT; ++ct) {
            const f32x4 y = tile_product<G::CIP, G::PX, G::PWO>(A, W, ct, lane);
            const int col = ct * 16 + c16;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool live = col < C && r0 + 4 * g + r < a.R;
                const float yc = (y[r] + bias.v[ct]) - mu.v[ct];
                const float xh = yc * is.v[ct];
                float gv = !live ? 0.f : vec ? T1[(4 * g + r) * G::PX + col] : a.dz[(size_t)(r0 + 4 * g + r) * a.lddz + col];
                if (__builtin_fmaf(yc, sc.v[ct], be.v[ct]) <= 0.f) gv *= 0.2f;
                const float dyv = live ? sc.v[ct] * (gv - m1.v[ct] - xh * m2.v[ct]) : 0.f;
                T1[(4 * g + r) * G::PX + col] = a.bf16 ? round_bf16(dyv) : dyv;  // (operand of the two products; the bias gradient sums the unrounded value)
                if (WG) dbs[ct] += dyv;
            }
        }
        wave_lds_sync();
        if (WG) xt_mma<NT, NT, G::PX, G::PX>(A, T1, dw, lane);  // dW += x^T dy
        if (vec) wave_lds_sync();  // the x tile is dead from here on: it stages dx
        // dx = dy . W^T
#pragma unroll
        for (int tj = 0; tj < NT; ++tj) {
            const f32x4 acc = tile_product<CP, G::PX, G::PWI>(T1, WT, tj, lane);
            const int col = tj * 16 + c16;
            if (vec) {
#pragma unroll
                for (int r = 0; r < 4; ++r) A[(4 * g + r) * G::PX + col] = acc[r];
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (col < C && r0 + 4 * g + r < a.R) {
                        float* dst = a.out + (size_t)(r0 + 4 * g + r) * a.ldo + col;
                        *dst = a.accum ? *dst + acc[r] : acc[r];
                    }
            }
        }
        wave_lds_sync();
        ScTile<C> o;
        if (vec) {
            o.take(A, lane);
            if (acc_old) old_cur.template expand<XB>(), o.add(old_cur);
            wave_lds_sync();
        }
        if (more) {
            xr.template expand<XB>(), xr.commit(A, lane, a.bf16 != 0);
            if (vec) zr.template expand<XB>(), zr.commit(T1, lane);
        }
        if (vec) o.template put_any<XB>(a.out, a.ldo, r0, a.R, lane);
        wave_lds_sync();
    }
    if (WG) {  // the workgroup's partial: waves add up through LDS in order (weights and tiles are dead)
        constexpr int NV = CP * CP + CP;
        __syncthreads();
        float* red = smem;
        float* r = red + (size_t)wave * NV;
        cols_to_lds(r + CP * CP, 0, lane, dbs), acc_to_lds(dw, r, CP, lane);
        wg_merge<float, kScWaves>(red, NV, static_cast<float*>(a.part) + (size_t)blockIdx.x * NV);
    }
}

static bool sc_ok(int64_t C) { return C == 8 || C == 16 || C == 32 || C == 64; }

// what: 0 forward sums, 1 forward apply, 2 backward sums (S1 | S2 | XS | A | G), 3 backward apply, 4 backward sums (S1 | S2 | XS only),
//       5 backward apply + weight / bias gradient (result = dW, result2 = db)
template <int C, bool XB>
static int sc_launch_x(ps_context* c, ScArgs a, int what, void* result, void* result2)
{
    using G = ScGeom<C>;
    constexpr int CP = G::COP, NVB = 3 * CP + 2 * CP * CP, NVW = CP * CP + CP;
    constexpr size_t wts = sizeof(float) * CP * G::PWO, tile = sizeof(float) * 16 * G::PX;
    void (*const kern[6])(ScArgs) = {sc_sums_kernel<C, XB>,           sc_apply_kernel<C, XB>,           sc_bwd_sums_kernel<C, true, XB>,
                                     sc_bwd_apply_kernel<C, false, XB>, sc_bwd_sums_kernel<C, false, XB>, sc_bwd_apply_kernel<C, true, XB>};
    const int nv[6] = {3 * CP, 0, NVB, 0, 3 * CP, NVW};  // values of a workgroup's partial (doubles for what = 0)
    const size_t lds[6] = {wts + kScWaves * tile + sizeof(double) * kScWaves * nv[0],
                           wts + kScWaves * tile,
                           std::max(wts + kScWaves * 3 * tile, sizeof(float) * (size_t)kScWaves * nv[2]),
                           2 * wts + kScWaves * 2 * tile,
                           std::max(wts + kScWaves * 3 * tile, sizeof(float) * (size_t)kScWaves * nv[4]),
                           std::max(2 * wts + kScWaves * 2 * tile, sizeof(float) * (size_t)kScWaves * nv[5])};
    const size_t smem = lds[what];
    PS_CHECK(smem <= 160 * 1024, "smallconv_train: %zu bytes of LDS needed", smem);
    const int blocks = convbn_blocks(a.R, kScWaves, smem), n = nv[what];
    if (n) {
        PS_TRY(c->red_ws.reserve((what == 0 ? sizeof(double) : sizeof(float)) * (size_t)blocks * n + 256));
        a.part = c->red_ws.as<void>();
    }
    PS_TRY(convbn_launch(c, kern[what], blocks, kScWaves * 64, smem, a));
    if (what == 0)
        hipLaunchKernelGGL(reduce_partials_kernel<double>, dim3(ceil_div(n, 16)), dim3(256), 0, c->stream, static_cast<const double*>(a.part), blocks, n,
                           static_cast<double*>(result));
    else if (what == 2 || what == 4)
        hipLaunchKernelGGL(reduce_partials_kernel<float>, dim3(ceil_div(n, 16)), dim3(256), 0, c->stream, static_cast<const float*>(a.part), blocks, n,
                           static_cast<float*>(result));
    else if (what == 5)
        hipLaunchKernelGGL(reduce_partials2_kernel<float>, dim3(ceil_div(n, 16)), dim3(256), 0, c->stream, static_cast<const float*>(a.part), blocks, n, CP * CP,
                           static_cast<float*>(result), static_cast<float*>(result2));
    PS_HIP(hipGetLastError());
    return PS_OK;
}

template <int C>
static int sc_launch(ps_context* c, const ScArgs& a, int what, void* result, void* result2 = nullptr)
{
    return a.x_bf16 ? sc_launch_x<C, true>(c, a, what, result, result2) : sc_launch_x<C, false>(c, a, what, result, result2);
}

static int sc_dispatch(ps_context* c, int64_t C, const ScArgs& a_in, int what, void* result, void* result2 = nullptr)
{
    ScArgs a = a_in;
    auto al = [](const void* q, int ld) { return !q || ((reinterpret_cast<uintptr_t>(q) & 15) == 0 && ld % 4 == 0); };
    a.vec = al(a.dz, a.lddz) && al(a.out, a.ldo) ? 1 : 0;
    PS_CHECK(!a.x_bf16 || a.vec, "ps_op_conv_bn_train_*: bfloat16 rows (x, the output, dz, dx: ps_set_train_act_bf16) need 16-byte aligned bases and pitches %% 4 == 0");
    a.bf16 = c->train_bf16 && C % 16 == 0 ? 1 : 0;  // (ps_set_train_gemm_bf16; the rule of ps_op_conv1x1_ex: an 8-channel product stays fp32)
    switch (C) {
        case 8: return sc_launch<8>(c, a, what, result, result2);
        case 16: return sc_launch<16>(c, a, what, result, result2);
        case 32: return sc_launch<32>(c, a, what, result, result2);
        default: return sc_launch<64>(c, a, what, result, result2);
    }
}

// one thread per row at C = 8 (convbn_rows.hip)
int convbn_rows_sums(ps_context* c, const float* x, int64_t ldx, const float* w, const float* b, int64_t R, double* sums);
int convbn_rows_apply(ps_context* c, const float* x, int64_t ldx, const float* w, const float* b, int64_t R, const float* mean, const float* scale,
                      const float* beta, float* out, int64_t ldo);
int convbn_rows_bwd_sums(ps_context* c, const float* x, int64_t ldx, const float* w, const float* b, int64_t R, const float* mean, const float* invstd,
                         const float* scale, const float* beta, const float* dz, int64_t lddz, float* s12);
int convbn_rows_bwd_apply(ps_context* c, const float* x, int64_t ldx, const float* w, const float* b, int64_t R, const float* mean, const float* invstd,
                          const float* scale, const float* beta, const float* s12, float inv_rows, const float* dz, int64_t lddz, int accumulate, float* dx,
                          int64_t lddx, float* dw, float* db);

// what every entry starts from
static ScArgs sc_args(const ps_context* c, const float* x, int64_t ldx, const float* w, const float* b, int64_t R)
{
    ScArgs a = {};
    a.x_bf16 = convbn_rows_bf16(c) ? 1 : 0;
    a.x = x; a.ldx = (int)ldx; a.w = w; a.b = b; a.R = R;
    return a;
}

}  // namespace ps

using namespace ps;

extern "C" int ps_op_conv_bn_train_supported(int64_t C) { return sc_ok(C) ? 1 : 0; }

extern "C" int ps_op_conv_bn_train_sums(ps_context* c, const float* x, int64_t ldx, const float* w, const float* b, int64_t R, int64_t C, double* sums)
{
    PS_CHECK(c && w && b && sums && sc_ok(C) && rows_ok(x, ldx, C), "ps_op_conv_bn_train_sums: C in {8, 16, 32, 64}, rows 16-byte aligned");
    PS_HIP(hipSetDevice(c->device));
    const int64_t CP = C < 16 ? 16 : C;
    if (R <= 0) {
        PS_HIP(hipMemsetAsync(sums, 0, sizeof(double) * 3 * CP, c->stream));
        return PS_OK;
    }
    Stage st(c, "train_convbn_fwd", 2);
    if (C == 8) return convbn_rows_sums(c, x, ldx, w, b, R, sums);
    return sc_dispatch(c, C, sc_args(c, x, ldx, w, b, R), 0, sums);
}

extern "C" int ps_op_conv_bn_train_apply(ps_context* c, const float* x, int64_t ldx, const float* w, const float* b, int64_t R, int64_t C, const float* mean,
                                         const float* scale, const float* beta, float* out, int64_t ldo)
{
    PS_CHECK(c && w && b && mean && scale && beta && out && sc_ok(C) && rows_ok(x, ldx, C) && ldo >= C,
             "ps_op_conv_bn_train_apply: C in {8, 16, 32, 64}, rows 16-byte aligned");
    if (R <= 0) return PS_OK;
    PS_HIP(hipSetDevice(c->device));
    Stage st(c, "train_convbn_fwd", 1);
    if (C == 8 && ldo % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0) return convbn_rows_apply(c, x, ldx, w, b, R, mean, scale, beta, out, ldo);
    ScArgs a = sc_args(c, x, ldx, w, b, R);
    a.mean = mean; a.scale = scale; a.beta = beta; a.out = out; a.ldo = (int)ldo;
    return sc_dispatch(c, C, a, 1, nullptr);
}

extern "C" int ps_op_conv_bn_train_bwd_sums(ps_context* c, const float* x, int64_t ldx, const float* w, const float* b, int64_t R, int64_t C,
                                            const float* mean, const float* invstd, const float* scale, const float* beta, const float* dz, int64_t lddz,
                                            float* sums)
{
    PS_CHECK(c && w && b && mean && invstd && scale && beta && dz && sums && sc_ok(C) && rows_ok(x, ldx, C) && lddz >= C,
             "ps_op_conv_bn_train_bwd_sums: C in {8, 16, 32, 64}, rows 16-byte aligned");
    PS_HIP(hipSetDevice(c->device));
    const int64_t CP = C < 16 ? 16 : C;
    if (R <= 0) {
        PS_HIP(hipMemsetAsync(sums, 0, sizeof(float) * (3 * CP + 2 * CP * CP), c->stream));
        return PS_OK;
    }
    Stage st(c, "train_convbn_bwd", 2);
    ScArgs a = sc_args(c, x, ldx, w, b, R);
    a.mean = mean; a.invstd = invstd; a.scale = scale; a.beta = beta; a.dz = dz; a.lddz = (int)lddz;
    return sc_dispatch(c, C, a, 2, sums);
}

extern "C" int ps_op_conv_bn_train_bwd_apply(ps_context* c, const float* x, int64_t ldx, const float* w, const float* b, int64_t R, int64_t C,
                                             const float* mean, const float* invstd, const float* scale, const float* beta, const float* m1,
                                             const float* m2, const float* dz, int64_t lddz, int accumulate, float* dx, int64_t lddx)
{
    PS_CHECK(c && w && b && mean && invstd && scale && beta && m1 && m2 && dz && dx && sc_ok(C) && rows_ok(x, ldx, C) && lddz >= C && lddx >= C,
             "ps_op_conv_bn_train_bwd_apply: C in {8, 16, 32, 64}, rows 16-byte aligned");
    if (R <= 0) return PS_OK;
    PS_HIP(hipSetDevice(c->device));
    Stage st(c, "train_convbn_bwd", 1);
    ScArgs a = sc_args(c, x, ldx, w, b, R);
    a.mean = mean; a.invstd = invstd; a.scale = scale; a.beta = beta; a.m1 = m1; a.m2 = m2;
    a.dz = dz; a.lddz = (int)lddz; a.out = dx; a.ldo = (int)lddx; a.accum = accumulate ? 1 : 0; a.mscale = 1.f;
    return sc_dispatch(c, C, a, 3, nullptr);
}

extern "C" int ps_op_conv_bn_train_bwd_sums2(ps_context* c, const float* x, int64_t ldx, const float* w, const float* b, int64_t R, int64_t C,
                                             const float* mean, const float* invstd, const float* scale, const float* beta, const float* dz, int64_t lddz,
                                             float* s12)
{
    PS_CHECK(c && w && b && mean && invstd && scale && beta && dz && s12 && sc_ok(C) && rows_ok(x, ldx, C) && lddz >= C,
             "ps_op_conv_bn_train_bwd_sums2: C in {8, 16, 32, 64}, rows 16-byte aligned");
    PS_HIP(hipSetDevice(c->device));
    if (R <= 0) {
        PS_HIP(hipMemsetAsync(s12, 0, sizeof(float) * 3 * C, c->stream));
        return PS_OK;
    }
    Stage st(c, "train_convbn_bwd", 2);
    if (C == 8 && rows_ok(dz, lddz, C)) return convbn_rows_bwd_sums(c, x, ldx, w, b, R, mean, invstd, scale, beta, dz, lddz, s12);
    PS_CHECK(C >= 16, "ps_op_conv_bn_train_bwd_sums2: C = 8 needs 16-byte aligned dz rows");
    ScArgs a = sc_args(c, x, ldx, w, b, R);
    a.mean = mean; a.invstd = invstd; a.scale = scale; a.beta = beta; a.dz = dz; a.lddz = (int)lddz;
    return sc_dispatch(c, C, a, 4, s12);
}

extern "C" int ps_op_conv_bn_train_bwd_apply_w(ps_context* c, const float* x, int64_t ldx, const float* w, const float* b, int64_t R, int64_t C,
                                               const float* mean, const float* invstd, const float* scale, const float* beta, const float* s12,
                                               float inv_rows, const float* dz, int64_t lddz, int accumulate, float* dx, int64_t lddx, float* dw, float* db)
{
    PS_CHECK(c && w && b && mean && invstd && scale && beta && s12 && dz && dx && dw && db && sc_ok(C) && rows_ok(x, ldx, C) && lddz >= C && lddx >= C,
             "ps_op_conv_bn_train_bwd_apply_w: C in {8, 16, 32, 64}, rows 16-byte aligned");
    PS_HIP(hipSetDevice(c->device));
    if (R <= 0) {
        PS_HIP(hipMemsetAsync(dw, 0, sizeof(float) * C * C, c->stream));
        PS_HIP(hipMemsetAsync(db, 0, sizeof(float) * C, c->stream));
        return PS_OK;
    }
    Stage st(c, "train_convbn_bwd", 2);
    if (C == 8 && rows_ok(dz, lddz, C) && rows_ok(dx, lddx, C))
        return convbn_rows_bwd_apply(c, x, ldx, w, b, R, mean, invstd, scale, beta, s12, inv_rows, dz, lddz, accumulate, dx, lddx, dw, db);
    PS_CHECK(C >= 16, "ps_op_conv_bn_train_bwd_apply_w: C = 8 needs 16-byte aligned dz / dx rows");
    ScArgs a = sc_args(c, x, ldx, w, b, R);
    a.mean = mean; a.invstd = invstd; a.scale = scale; a.beta = beta; a.m1 = s12; a.m2 = s12 + C;
    a.mscale = inv_rows; a.dz = dz; a.lddz = (int)lddz; a.out = dx; a.ldo = (int)lddx; a.accum = accumulate ? 1 : 0;
    return sc_dispatch(c, C, a, 5, dw, db);
}
