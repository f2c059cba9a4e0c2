// rectconv_train.hip -- conv2d(cin -> cout) + batch_normalization(training=True) [+ LeakyReLU] of the TRAINING step on [N]-row tensors with the
// pre-BatchNorm product recomputed instead of stored, for cin != cout.  The tile mechanics (geometry, the tile's way global -> registers -> LDS
// and back, weight staging, the two MFMA loops, the workgroup tail) are convbn_tile.h's, shared with smallconv_train.hip (c -> c); this
// file's own: the optional activation (leaky), the residual addend (ADD), the optional dx, and 4 or 8 waves per workgroup.
//
//   The shared MLPs that WIDEN their rows -- Encoder mlp2 (d -> 2d) and shortcut (d_in -> 2d) of dilated_res_block (RandLANet.py:312-321, no
//   activation: the sum gets it), fc1 of the head (32 -> 64, :145) -- at the point counts of levels 0-1 of a batch of 8 x 180 000 points.
//   Op by op such a layer makes 3 passes over its input width and 11 over its OUTPUT width (product written, read for the statistics, read
//   and written normalised; BatchNorm backward 2 + 3; input gradient 1; weight gradient 1); recomputed from 16-row tiles of x on the fp32
//   MFMA it is 5 passes over the input width and 3 over the output width -- for 16 -> 32 channels 11 units instead of 25.
//     forward   sums      : sum y, sum y^2 per output channel (fp64)                                            reads x
//               apply     : z = act((y - mean) gamma invstd + beta)                                              reads x, writes z
//     backward  sums      : g = dz act'(.), xh = (y - mean) invstd:  S1 = sum g, S2 = sum g xh                   reads x, dz
//               apply     : dy = gamma invstd (g - S1/M - xh S2/M);  dx (+)= dy . W^T;  dW = x^T dy, db = sum dy  reads x, dz, writes dx
//   Tiles travel as 16-byte accesses fetched one tile ahead and staged through LDS (the lesson of smallconv_train.hip's first form).  Sums are
//   per-workgroup partials merged in a fixed order (deterministic).  bf16-MLP mode: the operands of the three products are rounded to
//   bfloat16 first (cin % 16 == 0, the rule of ps_op_conv1x1_ex).  Compiled pairs: ps_op_convbn_train_supported.
#include "convbn_tile.h"
#include "reduce_partials.h"

namespace ps {

struct RcArgs {
    const float* x;      // [R, CI] rows (ldx)
    const float* w;      // [CI, CO] row-major
    const float* b;      // [CO]
    const float* mean; const float* invstd; const float* scale; const float* beta;  // [CO]; scale = gamma invstd
    const float* s12;    // [2 CO] S1 | S2 of all ranks (backward apply)
    float inv_rows;      // 1 / rows of all ranks
    const float* dz;     // [R, CO] (lddz)
    float* out;          // apply: z rows [R, CO];  backward apply: dx rows [R, CI]  (ldo)
    void* part;          // per-workgroup partial sums
    int64_t R;
    int ldx, lddz, ldo, accum, leaky, bf16;
    const float* addend;  // apply: non-null -> out = LeakyReLU(BN(x . W + b) + addend) (rows [R, CO], ld_add): the residual sum of dilated_res_block
    int ld_add;          // (RandLANet.py:306-307) in the pass that writes the second summand instead of a pass of its own
};

// the geometry of convbn_tile.h and this file's waves per workgroup (LDS: both weight orientations + two tiles per wave)
template <int CI, int CO>
struct RcGeom : ConvGeom<CI, CO> {
    static constexpr int WAVES = ConvGeom<CI, CO>::CIP * ConvGeom<CI, CO>::COP >= 4096 ? 4 : 8;
};

// ---- forward: statistics.  partial per workgroup (doubles): sy[COP] | sq[COP]
template <int CI, int CO>
__global__ __launch_bounds__((RcGeom<CI, CO>::WAVES * 64)) void rc_sums_kernel(RcArgs a)
{
    using G = RcGeom<CI, CO>;
    constexpr int kRcWaves = G::WAVES;
    constexpr int NT = G::NTO;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* W = smem;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, g = lane >> 4, c16 = lane & 15;
    float* X = smem + G::CIP * G::PWO + wave * 16 * G::PX;
    double* red = reinterpret_cast<double*>(smem + G::CIP * G::PWO + kRcWaves * 16 * G::PX);  // [kRcWaves][2 COP]
    stage_w<CI, CO, kRcWaves * 64>(a.w, W, nullptr, a.bf16 != 0);
    __syncthreads();
    const Cols<NT> bias(a.b, c16, CO);
    double sy[NT], sq[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) { sy[t] = 0.; sq[t] = 0.; }
    const int64_t tiles = (a.R + 15) / 16, tstride = (int64_t)gridDim.x * kRcWaves;
    int64_t tl = (int64_t)blockIdx.x * kRcWaves + wave;
    RowTile<CI, G::PX> xr;
    if (tl < tiles) xr.fetch(a.x, a.ldx, tl * 16, a.R, lane);
    for (; tl < tiles; tl += tstride) {
        const int64_t r0 = tl * 16;
        xr.commit(X, lane, a.bf16 != 0);
        wave_lds_sync();
        if (tl + tstride < tiles) xr.fetch(a.x, a.ldx, (tl + tstride) * 16, a.R, lane);
#pragma unroll
        for (int ct = 0; ct < NT; ++ct) {
            const f32x4 y = tile_product<G::CIP, G::PX, G::PWO>(X, W, ct, lane);
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (r0 + 4 * g + r < a.R) {
                    const double yd = (double)(y[r] + bias.v[ct]);
                    sy[ct] += yd;
                    sq[ct] = __builtin_fma(yd, yd, sq[ct]);
                }
        }
        wave_lds_sync();
    }
    cols_to_lds(red + wave * 2 * G::COP, G::COP, lane, sy, sq);
    wg_merge<double, kRcWaves>(red, 2 * G::COP, static_cast<double*>(a.part) + (size_t)blockIdx.x * 2 * G::COP);
}

// ---- forward: normalise (+ LeakyReLU) -> rows.  ADD: + addend rows, then LeakyReLU (a template parameter: a run-time branch around the addend
// tile's prefetch would make the compiler wait for every load in flight at the join)
template <int CI, int CO, bool ADD>
__global__ __launch_bounds__((RcGeom<CI, CO>::WAVES * 64)) void rc_apply_kernel(RcArgs a)
{
    using G = RcGeom<CI, CO>;
    constexpr int kRcWaves = G::WAVES;
    constexpr int NT = G::NTO;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* W = smem;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, g = lane >> 4, c16 = lane & 15;
    float* X = smem + G::CIP * G::PWO + wave * 16 * (G::PX + G::PZ);
    float* Z = X + 16 * G::PX;
    stage_w<CI, CO, kRcWaves * 64>(a.w, W, nullptr, a.bf16 != 0);
    __syncthreads();
    const Cols<NT> bias(a.b, c16, CO), mu(a.mean, c16, CO), sc(a.scale, c16, CO), be(a.beta, c16, CO);
    const int64_t tiles = (a.R + 15) / 16, tstride = (int64_t)gridDim.x * kRcWaves;
    int64_t tl = (int64_t)blockIdx.x * kRcWaves + wave;
    RowTile<CI, G::PX> xr;
    RowTile<CO, G::PZ> ad;
    if (tl < tiles) {
        xr.fetch(a.x, a.ldx, tl * 16, a.R, lane);
        if constexpr (ADD) ad.fetch(a.addend, a.ld_add, tl * 16, a.R, lane);
    }
    for (; tl < tiles; tl += tstride) {
        const int64_t r0 = tl * 16;
        xr.commit(X, lane, a.bf16 != 0);
        wave_lds_sync();
        [[maybe_unused]] const RowTile<CO, G::PZ> ad_cur = ad;
        if (tl + tstride < tiles) {
            xr.fetch(a.x, a.ldx, (tl + tstride) * 16, a.R, lane);
            if constexpr (ADD) ad.fetch(a.addend, a.ld_add, (tl + tstride) * 16, a.R, lane);
        }
#pragma unroll
        for (int ct = 0; ct < NT; ++ct) {
            const f32x4 y = tile_product<G::CIP, G::PX, G::PWO>(X, W, ct, lane);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float t = __builtin_fmaf((y[r] + bias.v[ct]) - mu.v[ct], sc.v[ct], be.v[ct]);
                if (a.leaky && t < 0.f) t *= 0.2f;
                Z[(4 * g + r) * G::PZ + ct * 16 + c16] = t;
            }
        }
        wave_lds_sync();
        RowTile<CO, G::PZ> o;
        o.take(Z, lane);
        if constexpr (ADD) {
            o.add(ad_cur);
            o.lrelu();
        }
        o.put(a.out, a.ldo, r0, a.R, lane);
        wave_lds_sync();
    }
}

// ---- backward: S1 = sum g, S2 = sum g xh.  partial per workgroup (floats): S1[COP] | S2[COP]
template <int CI, int CO>
__global__ __launch_bounds__((RcGeom<CI, CO>::WAVES * 64)) void rc_bwd_sums_kernel(RcArgs a)
{
    using G = RcGeom<CI, CO>;
    constexpr int kRcWaves = G::WAVES;
    constexpr int NT = G::NTO, COP = G::COP;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* W = smem;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, g = lane >> 4, c16 = lane & 15;
    float* X = smem + G::CIP * G::PWO + wave * 16 * (G::PX + G::PZ);
    float* Z = X + 16 * G::PX;
    float* red = smem + G::CIP * G::PWO + kRcWaves * 16 * (G::PX + G::PZ);  // [kRcWaves][2 COP]
    stage_w<CI, CO, kRcWaves * 64>(a.w, W, nullptr, a.bf16 != 0);
    __syncthreads();
    const Cols<NT> bias(a.b, c16, CO), mu(a.mean, c16, CO), is(a.invstd, c16, CO), sc(a.scale, c16, CO), be(a.beta, c16, CO);
    float s1[NT], s2[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) { s1[t] = 0.f; s2[t] = 0.f; }
    const int64_t tiles = (a.R + 15) / 16, tstride = (int64_t)gridDim.x * kRcWaves;
    int64_t tl = (int64_t)blockIdx.x * kRcWaves + wave;
    RowTile<CI, G::PX> xr;
    RowTile<CO, G::PZ> zr;
    if (tl < tiles) {
        xr.fetch(a.x, a.ldx, tl * 16, a.R, lane);
        zr.fetch(a.dz, a.lddz, tl * 16, a.R, lane);
    }
    for (; tl < tiles; tl += tstride) {
        const int64_t r0 = tl * 16;
        xr.commit(X, lane, a.bf16 != 0);
        zr.commit(Z, lane, false);
        wave_lds_sync();
        if (tl + tstride < tiles) {
            xr.fetch(a.x, a.ldx, (tl + tstride) * 16, a.R, lane);
            zr.fetch(a.dz, a.lddz, (tl + tstride) * 16, a.R, lane);
        }
#pragma unroll
        for (int ct = 0; ct < NT; ++ct) {
            const f32x4 y = tile_product<G::CIP, G::PX, G::PWO>(X, W, ct, lane);
            const int col = ct * 16 + c16;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool live = col < CO && r0 + 4 * g + r < a.R;
                const float yc = (y[r] + bias.v[ct]) - mu.v[ct];
                const float xh = live ? yc * is.v[ct] : 0.f;
                float gv = live ? Z[(4 * g + r) * G::PZ + col] : 0.f;
                if (a.leaky && __builtin_fmaf(yc, sc.v[ct], be.v[ct]) <= 0.f) gv *= 0.2f;
                s1[ct] += gv;
                s2[ct] = __builtin_fmaf(gv, xh, s2[ct]);
            }
        }
        wave_lds_sync();
    }
    cols_to_lds(red + wave * 2 * COP, COP, lane, s1, s2);
    wg_merge<float, kRcWaves>(red, 2 * COP, static_cast<float*>(a.part) + (size_t)blockIdx.x * 2 * COP);
}

// ---- backward: input gradient rows + weight / bias gradient.  partial per workgroup (floats): dW[CIP][COP] | db[COP]
template <int CI, int CO>
__global__ __launch_bounds__((RcGeom<CI, CO>::WAVES * 64)) void rc_bwd_apply_kernel(RcArgs a)
{
    using G = RcGeom<CI, CO>;
    constexpr int kRcWaves = G::WAVES;
    constexpr int NTI = G::NTI, NTO = G::NTO, CIP = G::CIP, COP = G::COP, NV = CIP * COP + COP;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* W = smem;
    float* WT = smem + CIP * G::PWO;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, g = lane >> 4, c16 = lane & 15;
    float* X = smem + CIP * G::PWO + COP * G::PWI + wave * 16 * (G::PX + G::PZ);
    float* Z = X + 16 * G::PX;  // dz, replaced in place by dy
    stage_w<CI, CO, kRcWaves * 64>(a.w, W, WT, a.bf16 != 0);
    __syncthreads();
    const Cols<NTO> bias(a.b, c16, CO), mu(a.mean, c16, CO), is(a.invstd, c16, CO), sc(a.scale, c16, CO), be(a.beta, c16, CO);
    const Cols<NTO> m1(a.s12, c16, CO, a.inv_rows), m2(a.s12 + CO, c16, CO, a.inv_rows);
    f32x4 dw[NTI][NTO];
    float dbs[NTO];
#pragma unroll
    for (int u = 0; u < NTO; ++u) {
        dbs[u] = 0.f;
#pragma unroll
        for (int t = 0; t < NTI; ++t) dw[t][u] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const int64_t tiles = (a.R + 15) / 16, tstride = (int64_t)gridDim.x * kRcWaves;
    int64_t tl = (int64_t)blockIdx.x * kRcWaves + wave;
    const bool want_dx = a.out != nullptr, acc_old = want_dx && a.accum;
    RowTile<CI, G::PX> xr, old_next;
    RowTile<CO, G::PZ> zr;
    if (tl < tiles) {
        xr.fetch(a.x, a.ldx, tl * 16, a.R, lane);
        zr.fetch(a.dz, a.lddz, tl * 16, a.R, lane);
        if (acc_old) old_next.fetch(a.out, a.ldo, tl * 16, a.R, lane);
        xr.commit(X, lane, a.bf16 != 0);
        zr.commit(Z, lane, false);
    }
    wave_lds_sync();
    for (; tl < tiles; tl += tstride) {
        const int64_t r0 = tl * 16;
        const bool more = tl + tstride < tiles;
        RowTile<CI, G::PX> old_cur = old_next;
        if (more) {
            xr.fetch(a.x, a.ldx, (tl + tstride) * 16, a.R, lane);
            zr.fetch(a.dz, a.lddz, (tl + tstride) * 16, a.R, lane);
            if (acc_old) old_next.fetch(a.out, a.ldo, (tl + tstride) * 16, a.R, lane);
        }
#pragma unroll
        for (int ct = 0; ct < NTO; ++ct) {
            const f32x4 y = tile_product<G::CIP, G::PX, G::PWO>(X, W, ct, lane);
            const int col = ct * 16 + c16;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool live = col < CO && r0 + 4 * g + r < a.R;
                const float yc = (y[r] + bias.v[ct]) - mu.v[ct];
                const float xh = yc * is.v[ct];
                float gv = live ? Z[(4 * g + r) * G::PZ + col] : 0.f;
                if (a.leaky && __builtin_fmaf(yc, sc.v[ct], be.v[ct]) <= 0.f) gv *= 0.2f;
                const float dyv = live ? sc.v[ct] * (gv - m1.v[ct] - xh * m2.v[ct]) : 0.f;
                Z[(4 * g + r) * G::PZ + col] = a.bf16 ? round_bf16(dyv) : dyv;  // (operand of the two products; db sums the unrounded value)
                dbs[ct] += dyv;
            }
        }
        wave_lds_sync();
        xt_mma<NTI, NTO, G::PX, G::PZ>(X, Z, dw, lane);  // dW += x^T dy
        RowTile<CI, G::PX> o;
        if (want_dx) {
            wave_lds_sync();  // the x tile is dead from here on: it stages dx
#pragma unroll
            for (int ti = 0; ti < NTI; ++ti) {  // dx = dy . W^T
                const f32x4 acc = tile_product<COP, G::PZ, G::PWI>(Z, WT, ti, lane);
#pragma unroll
                for (int r = 0; r < 4; ++r) X[(4 * g + r) * G::PX + ti * 16 + c16] = acc[r];
            }
            wave_lds_sync();
            o.take(X, lane);
            if (acc_old) o.add(old_cur);
        }
        wave_lds_sync();
        if (more) {
            xr.commit(X, lane, a.bf16 != 0);
            zr.commit(Z, lane, false);
        }
        if (want_dx) o.put(a.out, a.ldo, r0, a.R, lane);
        wave_lds_sync();
    }
    // the workgroup's partial: waves add up through LDS in order (weights and tiles are dead)
    __syncthreads();
    float* red = smem;
    float* r = red + (size_t)wave * NV;
    cols_to_lds(r + CIP * COP, 0, lane, dbs), acc_to_lds(dw, r, COP, lane);
    wg_merge<float, kRcWaves>(red, NV, static_cast<float*>(a.part) + (size_t)blockIdx.x * NV);
}

// dW partial [CIP][COP] | db[COP] (padded) -> dw [CI, CO], db [CO]
__global__ __launch_bounds__(256) void rc_unpad_kernel(const float* __restrict__ full, int CI, int CO, int COP, int CIPxCOP, float* __restrict__ dw,
                                                       float* __restrict__ db)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < CI * CO) dw[i] = full[(i / CO) * COP + i % CO];
    if (i < CO) db[i] = full[CIPxCOP + i];
}

// what: 0 forward sums, 1 forward apply, 2 backward sums, 3 backward apply (+ weight / bias gradient)
template <int CI, int CO>
static int rc_launch(ps_context* c, RcArgs a, int what, void* result, void* result2)
{
    using G = RcGeom<CI, CO>;
    constexpr int CIP = G::CIP, COP = G::COP, NVW = CIP * COP + COP, kRcWaves = G::WAVES;
    constexpr size_t w1 = sizeof(float) * CIP * G::PWO, w2 = sizeof(float) * COP * G::PWI;
    constexpr size_t tx = sizeof(float) * 16 * G::PX, tz = sizeof(float) * 16 * G::PZ;
    void (*const kern[4])(RcArgs) = {rc_sums_kernel<CI, CO>, a.addend ? rc_apply_kernel<CI, CO, true> : rc_apply_kernel<CI, CO, false>, rc_bwd_sums_kernel<CI, CO>,
                                     rc_bwd_apply_kernel<CI, CO>};
    const int nv[4] = {2 * COP, 0, 2 * COP, NVW};  // values of a workgroup's partial (doubles for what = 0)
    const size_t lds[4] = {w1 + kRcWaves * tx + sizeof(double) * kRcWaves * nv[0], w1 + kRcWaves * (tx + tz),
                           w1 + kRcWaves * (tx + tz) + sizeof(float) * kRcWaves * nv[2],
                           std::max(w1 + w2 + kRcWaves * (tx + tz), sizeof(float) * (size_t)kRcWaves * nv[3])};
    const size_t smem = lds[what];
    PS_CHECK(smem <= 160 * 1024, "rectconv_train: %zu bytes of LDS needed", smem);
    const int blocks = convbn_blocks(a.R, kRcWaves, smem), n = nv[what];
    if (n) {  // (what = 3: the partials, then their sum `full` behind them in the same workspace)
        PS_TRY(c->red_ws.reserve((what == 0 ? sizeof(double) : sizeof(float)) * ((size_t)blocks + (what == 3)) * n + 256));
        a.part = c->red_ws.as<void>();
    }
    PS_TRY(convbn_launch(c, kern[what], blocks, kRcWaves * 64, smem, a));
    if (what == 0) {
        hipLaunchKernelGGL(reduce_partials_kernel<double>, dim3(ceil_div(n, 16)), dim3(256), 0, c->stream, static_cast<const double*>(a.part), blocks, n,
                           static_cast<double*>(result));
    } else if (what == 2) {
        hipLaunchKernelGGL(reduce_partials_kernel<float>, dim3(ceil_div(n, 16)), dim3(256), 0, c->stream, static_cast<const float*>(a.part), blocks, n,
                           static_cast<float*>(result));
    } else if (what == 3) {  // ... then the unpadded copy into dw / db
        float* full = c->red_ws.as<float>() + (size_t)blocks * n;
        hipLaunchKernelGGL(reduce_partials_kernel<float>, dim3(ceil_div(n, 16)), dim3(256), 0, c->stream, static_cast<const float*>(a.part), blocks, n, full);
        hipLaunchKernelGGL(rc_unpad_kernel, dim3(ceil_div(std::max(CI * CO, CO), 256)), dim3(256), 0, c->stream, static_cast<const float*>(full), CI, CO, COP,
                           CIP * COP, static_cast<float*>(result), static_cast<float*>(result2));
    }
    PS_HIP(hipGetLastError());
    return PS_OK;
}

static bool rc_ok(int64_t ci, int64_t co)
{
    return (ci == 8 && co == 32) || (ci == 16 && co == 32) || (ci == 32 && co == 64) || (ci == 32 && co == 128) || (ci == 64 && co == 128);
}

static int rc_dispatch(ps_context* c, int64_t ci, int64_t co, RcArgs a, int what, void* result, void* result2 = nullptr)
{
    a.bf16 = c->train_bf16 && ci % 16 == 0 ? 1 : 0;  // (ps_set_train_gemm_bf16; the rule of ps_op_conv1x1_ex)
    if (ci == 8 && co == 32) return rc_launch<8, 32>(c, a, what, result, result2);
    if (ci == 16 && co == 32) return rc_launch<16, 32>(c, a, what, result, result2);
    if (ci == 32 && co == 64) return rc_launch<32, 64>(c, a, what, result, result2);
    if (ci == 32 && co == 128) return rc_launch<32, 128>(c, a, what, result, result2);
    return rc_launch<64, 128>(c, a, what, result, result2);
}

// what every entry starts from
static RcArgs rc_args(const float* x, int64_t ldx, const float* w, const float* b, int64_t R)
{
    RcArgs a = {};
    a.x = x; a.ldx = (int)ldx; a.w = w; a.b = b; a.R = R;
    return a;
}

}  // namespace ps

using namespace ps;

extern "C" int ps_op_convbn_train_supported(int64_t cin, int64_t cout) { return rc_ok(cin, cout) ? 1 : 0; }

extern "C" int ps_op_convbn_train_sums(ps_context* c, const float* x, int64_t ldx, const float* w, const float* b, int64_t R, int64_t cin, int64_t cout,
                                       double* sums)
{
    PS_CHECK(c && w && b && sums && rc_ok(cin, cout) && rows_ok(x, ldx, cin), "ps_op_convbn_train_sums: unsupported (cin, cout) or unaligned rows");
    PS_HIP(hipSetDevice(c->device));
    if (R <= 0) {
        PS_HIP(hipMemsetAsync(sums, 0, sizeof(double) * 2 * cout, c->stream));
        return PS_OK;
    }
    Stage st(c, "train_convbn_fwd", 2);
    return rc_dispatch(c, cin, cout, rc_args(x, ldx, w, b, R), 0, sums);
}

extern "C" int ps_op_convbn_train_apply(ps_context* c, const float* x, int64_t ldx, const float* w, const float* b, int64_t R, int64_t cin, int64_t cout,
                                        const float* mean, const float* scale, const float* beta, int leaky, float* out, int64_t ldo)
{
    PS_CHECK(c && w && b && mean && scale && beta && rc_ok(cin, cout) && rows_ok(x, ldx, cin) && rows_ok(out, ldo, cout),
             "ps_op_convbn_train_apply: unsupported (cin, cout) or unaligned rows");
    if (R <= 0) return PS_OK;
    PS_HIP(hipSetDevice(c->device));
    Stage st(c, "train_convbn_fwd", 1);
    RcArgs a = rc_args(x, ldx, w, b, R);
    a.mean = mean; a.scale = scale; a.beta = beta; a.leaky = leaky ? 1 : 0; a.out = out; a.ldo = (int)ldo;
    return rc_dispatch(c, cin, cout, a, 1, nullptr);
}

extern "C" int ps_op_convbn_train_apply_add(ps_context* c, const float* x, int64_t ldx, const float* w, const float* b, int64_t R, int64_t cin, int64_t cout,
                                            const float* mean, const float* scale, const float* beta, const float* addend, int64_t ld_add, float* out,
                                            int64_t ldo)
{
    PS_CHECK(c && w && b && mean && scale && beta && rc_ok(cin, cout) && rows_ok(x, ldx, cin) && rows_ok(out, ldo, cout) && rows_ok(addend, ld_add, cout),
             "ps_op_convbn_train_apply_add: unsupported (cin, cout) or unaligned rows");
    if (R <= 0) return PS_OK;
    PS_HIP(hipSetDevice(c->device));
    Stage st(c, "train_convbn_fwd", 1);
    RcArgs a = rc_args(x, ldx, w, b, R);
    a.mean = mean; a.scale = scale; a.beta = beta; a.leaky = 0; a.out = out; a.ldo = (int)ldo;
    a.addend = addend; a.ld_add = (int)ld_add;
    return rc_dispatch(c, cin, cout, a, 1, nullptr);
}

extern "C" int ps_op_convbn_train_bwd_sums(ps_context* c, const float* x, int64_t ldx, const float* w, const float* b, int64_t R, int64_t cin, int64_t cout,
                                           const float* mean, const float* invstd, const float* scale, const float* beta, int leaky, const float* dz,
                                           int64_t lddz, float* s12)
{
    PS_CHECK(c && w && b && mean && invstd && scale && beta && s12 && rc_ok(cin, cout) && rows_ok(x, ldx, cin) && rows_ok(dz, lddz, cout),
             "ps_op_convbn_train_bwd_sums: unsupported (cin, cout) or unaligned rows");
    PS_HIP(hipSetDevice(c->device));
    if (R <= 0) {
        PS_HIP(hipMemsetAsync(s12, 0, sizeof(float) * 2 * cout, c->stream));
        return PS_OK;
    }
    Stage st(c, "train_convbn_bwd", 2);
    RcArgs a = rc_args(x, ldx, w, b, R);
    a.mean = mean; a.invstd = invstd; a.scale = scale; a.beta = beta; a.leaky = leaky ? 1 : 0;
    a.dz = dz; a.lddz = (int)lddz;
    return rc_dispatch(c, cin, cout, a, 2, s12);
}

extern "C" int ps_op_convbn_train_bwd_apply(ps_context* c, const float* x, int64_t ldx, const float* w, const float* b, int64_t R, int64_t cin, int64_t cout,
                                            const float* mean, const float* invstd, const float* scale, const float* beta, int leaky, const float* s12,
                                            float inv_rows, const float* dz, int64_t lddz, int accumulate, float* dx, int64_t lddx, float* dw, float* db)
{
    PS_CHECK(c && w && b && mean && invstd && scale && beta && s12 && dw && db && rc_ok(cin, cout) && rows_ok(x, ldx, cin) && rows_ok(dz, lddz, cout) &&
                 (!dx || rows_ok(dx, lddx, cin)),
             "ps_op_convbn_train_bwd_apply: unsupported (cin, cout) or unaligned rows");
    PS_HIP(hipSetDevice(c->device));
    if (R <= 0) {
        PS_HIP(hipMemsetAsync(dw, 0, sizeof(float) * cin * cout, c->stream));
        PS_HIP(hipMemsetAsync(db, 0, sizeof(float) * cout, c->stream));
        return PS_OK;
    }
    Stage st(c, "train_convbn_bwd", 3);
    RcArgs a = rc_args(x, ldx, w, b, R);
    a.mean = mean; a.invstd = invstd; a.scale = scale; a.beta = beta; a.leaky = leaky ? 1 : 0;
    a.s12 = s12; a.inv_rows = inv_rows; a.dz = dz; a.lddz = (int)lddz; a.out = dx; a.ldo = (int)lddx; a.accum = accumulate ? 1 : 0;
    return rc_dispatch(c, cin, cout, a, 3, dw, db);
}
