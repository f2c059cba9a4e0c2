// attpool_gemm.hip -- attentive pooling of the TRAINING step at the wide levels (d = 128 / 256 / 512: encoder levels 2-4), forward and
// backward, with the score tensor never in memory.
//
//   att_pooling (PointSegment/RandLANet.py:388-398):   s = F . Wfc   (F = [N*K, d] neighbour set, no bias)
//                                                      p = softmax over the K rows of a point, per channel
//                                                      agg[n, c] = sum_k p[n,k,c] * F[n,k,c]
//
// attpool_train.hip fuses this per POINT with the d x d weights resident in LDS -- which ends at d = 64 in fp32 (d = 128 as bfloat16):
// the wide levels ran op by op (score GEMM -> s [N*K, d] -> softmax-pool kernel; backward: softmax-pool backward -> dS, dF -> input
// gradient GEMM -> weight gradient GEMM: fourteen passes over [N*K, d] tensors per pooling).  Here the two row-side products ride on
// gemm_b3.hip's frame instead -- v_mfma_f32_32x32x16_bf16 over exact three-way bfloat16 splits (P = 3: fp32 results) or one plane of
// rounded operands (P = 1: the bf16-MLP mode), the weight planes streamed L2 -> LDS in 24 KB blocks shared by the four waves of a
// workgroup -- and everything between them stays in the accumulator registers of the wave that owns the rows:
//
//   a wave owns 32 rows = the K = 16 neighbour rows of TWO points, all d columns, 128 columns (a "panel") at a time
//   forward    S = F . W (panel)            accumulator tile: lane = column, registers = rows -> a point's 16 scores of a channel are
//              8 registers of two lanes: softmax = in-lane + ONE v_permlane32_swap; agg = sum p F   -> only agg [N, d] is written
//   backward   S recomputed the same way;   dS = p g (F - agg),  direct = p g   (g = dagg of the point)
//              dS^T through the matrix pipe: T = dS^T . I (one MFMA per plane and 16 rows with an identity operand) turns the tile into
//              lane = row, registers = columns -- which IS the row operand of the next product, register for register (its K axis is
//              simply taken in accumulator order: the W^T image is packed to match, gemm_b3.hip b3_pack_elem<KMAP>) -- and the layout
//              in which a row of dS leaves as 16-byte stores;
//              dF = direct + dS . W^T       accumulated over the panels in registers, seeded with the direct term
//              -> reads F and dagg, writes dF and dS; the weight gradient dW = F^T . dS is the step's ordinary wgrad product over
//                 (F, dS) (wgrad_b3_kernel), whose d x d accumulators per row slab no row-owning wave could hold at d >= 256.
// Passes over [N*K, d] per pooling: forward 1 (was 4), backward 3 + 2 for dW (was 9).
//
// The steps the kernels share -- lane coordinates, the weight stream and its staging registers, the row source, the score product, the
// softmax / dS step, the transposing product, the dF tile stores -- are attpool_gemm_kit.h's; this file holds the three kernel bodies
// (what runs in which order) and the host side.
#include "attpool_gemm_kit.h"
#include "attpool_train.h"
#include "reduce_partials.h"

namespace ps {

template <int D, int P, bool SPLIT, bool FRB = false>
__global__ __launch_bounds__(256) void attg_fwd_kernel(AttGArgs a)
{
    static_assert(!FRB || (SPLIT && P == 1), "bfloat16 rows: split-source form of the bf16-MLP mode");
    using S = AttGStream<D, P, false>;
    __shared__ uint4 Bs[2][S::BLOCK];
    const AttGLane ln;
    const AttGRows rw = attg_rows(a, ln.wave);
    AttGSource<D, SPLIT, FRB> src(a, rw, ln);
    AttGStage<S> stg;
    stg.load(S::blk(a, 0));
    stg.store(Bs[0]);
    __syncthreads();
    int n = 0;
#pragma unroll 1
    for (int p = 0; p < S::NPAN; ++p) {
        f32x16 acc[4];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
        attg_scores<S>(a, src, stg, Bs, ln.lane, n, acc);
        // softmax over the 16 rows of each of the wave's two points, weighted sum of the value rows (the tile itself: L1 / L2 hits)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            __builtin_amdgcn_sched_barrier(0);  // (one tile's value loads at a time)
            const int col = 128 * p + 32 * t + ln.c32;
#pragma unroll
            for (int pi = 0; pi < 2; ++pi) {
                float fv[8];
                src.values(fv, col, pi);
                const AttGSoftmax sm = attg_softmax(acc[t], pi, fv);
                if (ln.hl == 0 && 16 * pi < rw.nvalid) a.agg[(size_t)((rw.rbase >> 4) + pi) * D + col] = sm.agg;
            }
        }
    }
}

// (d = 128: 64 + 64 accumulators leave room for two waves per SIMD -- asked for, the P = 1 form otherwise hoists its way past 256 registers;
//  d = 256 holds 64 + 128 accumulators: one wave per SIMD, the accumulators of dF in the second half of the register file)
//  d = 512 would hold 64 + 256: it runs as TWO launches, HALF = 0 / 1, each recomputing the scores and dS of every panel and accumulating
//  the dF columns of its half -- 64 + 128 accumulators like d = 256; dS is stored by the first)
template <int D, int P, bool SPLIT, int HALF = -1>
__global__ __launch_bounds__(256, D == 128 ? 2 : 1) void attg_bwd_kernel(AttGArgs a)
{
    static_assert(HALF < 0 || (D == 512 && !SPLIT), "the two-launch form is d = 512's");
    using S = AttGStream<D, P, true, HALF>;
    constexpr int NT = HALF < 0 ? D / 32 : D / 64, IT0 = HALF < 0 ? 0 : HALF * NT;  // dF tiles of this launch: IT0 .. IT0 + NT - 1
    __shared__ uint4 Bs[2][S::BLOCK];
    const AttGLane ln;
    const AttGRows rw = attg_rows(a, ln.wave);
    AttGSource<D, SPLIT, false> src(a, rw, ln);  // (bfloat16 rows: forward only)
    AttGStage<S> stg;
    const AttGTranspose tr(ln);
    f32x16 acc2[NT];  // dF of the wave's rows: tile it = columns 32 it .. (lane = column, registers = rows)
#pragma unroll
    for (int it = 0; it < NT; ++it)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc2[it][r] = 0.f;

    stg.load(S::blk(a, 0));
    stg.store(Bs[0]);
    __syncthreads();
    int n = 0;
    // (the panels through a compile-time index: `#pragma unroll` alone left the four-panel loop of d = 512 rolled at P = 3, and a run-time
    //  index into acc2 puts the dF accumulators into scratch memory)
    auto panel = [&](auto pc) __attribute__((always_inline)) {
        constexpr int p = decltype(pc)::value;
        f32x16 acc[4];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
        attg_scores<S>(a, src, stg, Bs, ln.lane, n, acc);
        // ---- softmax, direct term p g into the dF accumulators, dS = p g (F - agg) over the scores in place ----
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            __builtin_amdgcn_sched_barrier(0);  // (one tile's value loads at a time)
            const int col = 128 * p + 32 * t + ln.c32;
#pragma unroll
            for (int pi = 0; pi < 2; ++pi) {
                float fv[8];
                src.values(fv, col, pi);
                const float g = 16 * pi < rw.nvalid ? a.dagg[(size_t)((rw.rbase >> 4) + pi) * D + col] : 0.f;
                if constexpr (4 * p >= IT0 && 4 * p < IT0 + NT) {
                    attg_softmax_bwd<true>(acc[t], acc2[4 * p + t - IT0], pi, fv, g);
                } else {  // (two-launch form: the panel's dF columns are the other launch's)
                    f32x16 none;
                    attg_softmax_bwd<false>(acc[t], none, pi, fv, g);
                }
            }
        }
        // ---- per 32-column tile of the panel: transpose dS on the matrix pipe, store its rows, dF += dS . W^T ----
        float* dsb = a.ds + (size_t)rw.rbase * a.ldds;  // wave-uniform
        const unsigned dsoff = (unsigned)(ln.c32 * a.ldds + 128 * p + ln.row0());
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            __builtin_amdgcn_sched_barrier(0);
            const f32x16 T = tr.transposed<P>(acc[t]);  // lane = row c32 of the wave, register r = column 128 p + 32 t + row0() + attg_acc_row(r)
            if (HALF <= 0 && ln.c32 < rw.nvalid) {      // (two-launch form: the first launch stores dS)
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4)
                    *reinterpret_cast<float4*>(dsb + (dsoff + (unsigned)(32 * t + 8 * g4))) = make_float4(T[4 * g4], T[4 * g4 + 1], T[4 * g4 + 2], T[4 * g4 + 3]);
            }
            const BPlanes<P> tp[2] = {attg_tile_planes<P>(T, 0), attg_tile_planes<P>(T, 1)};
#pragma unroll
            for (int ig = 0; ig < S::NIG; ++ig, ++n) {
                const int buf = n & 1;
                const bool more = n + 1 < S::NB;
                if (more) stg.load(S::blk(a, n + 1));
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < 2; ++u)
#pragma unroll
                    for (int i4 = 0; i4 < 4; ++i4) {
                        BPlanes<P> bp;
#pragma unroll
                        for (int pl = 0; pl < P; ++pl) bp.p[pl] = Bs[buf][((u * 4 + i4) * P + pl) * 64 + ln.lane];
                        acc2[4 * ig + i4] = b3_mfma6<P>(tp[u], bp, acc2[4 * ig + i4]);
                    }
                if (more) stg.store(Bs[buf ^ 1]);
                __syncthreads();
            }
        }
    };
    attg_static_for<S::NPAN>(panel);
    // ---- dF: tile it = columns 32 (IT0 + it) .. ----
#pragma unroll
    for (int it = 0; it < NT; ++it) {
        // split form: the gathered half (tiles below D/2) leaves as plain rows for the gather-reduction, the right half goes to df
        const bool left = SPLIT && 32 * it < D / 2;
        const int pitch = left ? a.ld_rows : a.lddf;
        float* dfb = (left ? a.dfl_rows : a.df) + (size_t)rw.rbase * pitch;  // wave-uniform
        attg_store_df(dfb, 32 * (IT0 + it) + ln.c32 - (SPLIT && !left ? D / 2 : 0), pitch, rw.nvalid, !left && a.df_accum != 0, acc2[it], ln);
    }
}

__global__ __launch_bounds__(256) void attg_pack_kernel(PackJob j)
{
    // (one matrix, outside a recorded step: the batched kernel's element function through a by-value job)
    PackJob jj = j;
    for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < jj.total; i += (int64_t)gridDim.x * 256) b3_pack_elem_any(jj, i);
}

static int attg_planes(ps_context* c, const float* w, int64_t d, bool transposed_kmap, const uint4** out)
{
    PackJob key = {};
    key.w = w;
    key.sk = transposed_kmap ? 1 : d;
    key.sn = transposed_kmap ? d : 1;
    key.kind = (c->train_bf16 ? 4 : 3) + (transposed_kmap ? 2 : 0);
    key.cin = (int)d; key.cout = (int)d;
    key.total = (int64_t)(d / 16) * (d / 32) * 64;
    bool launch = true;
    void* planes = pack_slot(c, key, (size_t)d * d * 6, launch);
    PS_CHECK(planes != nullptr, "att_pool_gemm: out of device memory for the weight planes");
    if (launch) {
        key.out = planes;
        hipLaunchKernelGGL(attg_pack_kernel, dim3(ceil_div(key.total, 256)), dim3(256), 0, c->stream, key);
        PS_HIP(hipGetLastError());
    }
    *out = static_cast<const uint4*>(planes);
    return PS_OK;
}

template <int D, int P, bool BWD, bool SPLIT>
static int launch_attg_k(ps_context* c, const AttGArgs& a)
{
    auto go = [&](auto kern) { hipLaunchKernelGGL(kern, dim3((unsigned)((a.rows + 127) / 128)), dim3(256), 0, c->stream, a); };
    if constexpr (BWD && D == 512) {
        // 64 + 256 accumulators do not fit a wave: two launches over halves of the dF columns (attg_bwd_kernel, HALF)
        go(attg_bwd_kernel<D, P, false, 0>);
        go(attg_bwd_kernel<D, P, false, 1>);
    } else if constexpr (BWD) {
        go(attg_bwd_kernel<D, P, SPLIT>);
    } else if (a.f_bf16) {
        PS_CHECK(SPLIT && D == 128, "att_pool_gemm: bfloat16 rows are taken by the split-source forward at d = 128 only");
        PS_CHECK(P == 1, "att_pool_gemm: bfloat16 rows belong to the bf16-MLP mode");
        if constexpr (SPLIT && D == 128 && P == 1) go(attg_fwd_kernel<D, 1, true, true>);
    } else {
        go(attg_fwd_kernel<D, P, SPLIT>);
    }
    PS_HIP(hipGetLastError());
    return PS_OK;
}
template <int D, int P>
static int launch_attg_p(ps_context* c, const AttGArgs& a, bool bwd)
{
    if constexpr (D < 512) {  // (d = 512: materialised form only)
        if (a.fl) return bwd ? launch_attg_k<D, P, true, true>(c, a) : launch_attg_k<D, P, false, true>(c, a);
    }
    return bwd ? launch_attg_k<D, P, true, false>(c, a) : launch_attg_k<D, P, false, false>(c, a);
}
template <int D>
static int launch_attg_d(ps_context* c, const AttGArgs& a, bool bwd)
{
    return c->train_bf16 ? launch_attg_p<D, 1>(c, a, bwd) : launch_attg_p<D, 3>(c, a, bwd);  // (one plane in the bf16-MLP mode, else three)
}
static int launch_attg(ps_context* c, const AttGArgs& a, int64_t d, bool bwd)
{
    switch (d) {
        case 128: return launch_attg_d<128>(c, a, bwd);
        case 256: return launch_attg_d<256>(c, a, bwd);
        default: return launch_attg_d<512>(c, a, bwd);
    }
}

// ---- d = 64 (encoder level 1) -----------------------------------------------------------------------------------------------------------
// 5.76 M neighbour rows per batch of 8 clouds: the level where the [N*K, d] tensors are largest and where attpool_train.hip's per-point
// kernels (fp32 MFMA 16x16x4, a wave per point) were bound by the matrix pipe: 0.63 ms forward / 1.71 ms backward per pooling for 0.74 GB
// read / 2.9 GB moved.  Same computation as the wide-level kernels above with what d = 64 allows on top:
//   * both weight images (W planes for the scores, W^T planes in accumulator K order for dF: 24 KB each at P = 3) stay in LDS for the
//     whole kernel -- no stream, no workgroup barrier: the four waves of a workgroup walk their 32-row tiles independently (persistent grid);
//   * the weight gradient dW = F^T . dS (a third product, contraction over the 32 rows of the tile) accumulates in 64 registers per
//     wave: its row operand is the tile's value rows in exactly the register order the softmax epilogue loads them in (lane = column,
//     k-slots = rows), its column operand the planes of dS the transposing product consumes anyway -- per-wave partials, summed by
//     reduce_partials_kernel in a fixed order (deterministic: the grid does not depend on the data);
//   * split-source form (RandLANet.py:326-333: F = [gather(f, idx) | f_xyz]): the gathered half is read through idx (row operand: the
//     lane's own row; value rows: two int4 index loads per point), its gradient leaves as plain rows for the gather-reduction.
//   * per tile the only global reads are the 32 operand rows (the gathered half through one index per lane) and dagg: the rows are
//     requested ONE TILE AHEAD (the index two tiles ahead) and go to a per-wave LDS tile as they are split, which is where the softmax
//     epilogue and the weight-gradient product read their column-wise "value rows" from (the first form read them from global memory a
//     second time, behind the scores: 6.4 us per tile of exposed latency, 0.56 ms per forward pooling).
template <int P, bool BWD, int WAVES, bool FRB>  // FRB: the f_xyz half is stored as bfloat16 (compile-time: a run-time branch around the
                                                 // prefetch made the compiler wait for every load in flight at the join)
__global__ __launch_bounds__(WAVES * 64) void attg64_kernel(AttTrainArgs a, const uint4* __restrict__ w1, const uint4* __restrict__ w2, float* __restrict__ dw_part)
{
    constexpr int NQ = 4, NT = 2, IMG = NQ * NT * P * 64;  // uint4 per weight image
    constexpr int PITCH = 68;                               // floats per row of the value tile: 16-byte rows, the two lane halves on disjoint banks
    extern __shared__ __attribute__((aligned(16))) uint4 Wl[];
    for (int i = threadIdx.x; i < IMG; i += WAVES * 64) {
        Wl[i] = w1[i];
        if constexpr (BWD) Wl[IMG + i] = w2[i];
    }
    __syncthreads();
    const uint4* W1 = Wl;
    const uint4* W2 = Wl + IMG;
    const AttGLane ln;
    const int wave = ln.wave, lane = ln.lane, hl = ln.hl, c32 = ln.c32;
    float* V = reinterpret_cast<float*>(Wl + (BWD ? 2 : 1) * IMG) + wave * (32 * PITCH);
    const bool split = a.fl != nullptr;
    const AttGTranspose tr(ln);
    f32x16 acc3[2][2];  // dW of this wave: tile (it, ct) = rows 32 it .., columns 32 ct .. (lane = column, registers = rows)
    if constexpr (BWD) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc3[i][j][r] = 0.f;
    }
    const int64_t rows = a.R * 16;
    const int64_t ntiles = (rows + 31) >> 5;
    const int64_t stride = (int64_t)gridDim.x * WAVES;
    // the operand row of this lane in tile `tile` (rows is a multiple of 16: the last tile may hold ONE point, whose rows are then read twice)
    auto my_row = [&](int64_t tile) {
        const int64_t row0 = tile << 5;
        return row0 + ln.operand_row(rows - row0 >= 32 ? 16 : 0);
    };
    float4 nrow[8];   // the NEXT tile's operand row of this lane: chunks q = 0..3 x two float4
    int nidx = 0;     // split form: the lane's gathered row of the tile after that
    auto fetch_idx = [&](int64_t tile) { if (split && tile < ntiles) nidx = a.idx[my_row(tile)]; };
    auto fetch_row = [&](int64_t tile) {
        if (tile >= ntiles) return;
        const int64_t row = my_row(tile);
        const float *pL, *pR;
        if (split) {
            pL = a.fl + (size_t)(((row >> 4) / a.n_q) * a.n_src + nidx) * a.ldl + 8 * hl;
            pR = a.f + (size_t)row * a.ld + 8 * hl;
        } else {
            pL = a.f + (size_t)row * a.ld + 8 * hl;
            pR = pL + 32;
        }
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            if (FRB && q >= 2) {  // the f_xyz half stored as bfloat16 (split form only): one 16-byte load for the lane's eight values
                // (kept as loaded: converting here would make the wave wait for its own prefetch; expanded where the chunk is consumed)
                const uint4 u = *reinterpret_cast<const uint4*>(reinterpret_cast<const unsigned short*>(a.f) + ((size_t)row * a.ld + 8 * hl + 16 * (q - 2)));
                nrow[2 * q] = make_float4(__uint_as_float(u.x), __uint_as_float(u.y), __uint_as_float(u.z), __uint_as_float(u.w));
                continue;
            }
            const float* src = q < 2 ? pL + 16 * q : pR + 16 * (q - 2);
            nrow[2 * q] = *reinterpret_cast<const float4*>(src);
            nrow[2 * q + 1] = *reinterpret_cast<const float4*>(src + 4);
        }
    };
    int64_t tile = (int64_t)blockIdx.x * WAVES + wave;
    fetch_idx(tile);
    fetch_row(tile);
    fetch_idx(tile + stride);
#pragma unroll 1
    for (; tile < ntiles; tile += stride) {
        const int64_t row0 = tile << 5;
        const int nvalid = rows - row0 >= 32 ? 32 : 16;
        float gd[2][2];  // dagg of (tile column block t, point pi): requested before the products
        if constexpr (BWD) {
#pragma unroll
            for (int pi = 0; pi < 2; ++pi)
#pragma unroll
                for (int t = 0; t < 2; ++t)
                    gd[t][pi] = 16 * pi < nvalid ? a.dagg[(size_t)((row0 >> 4) + pi) * 64 + 32 * t + c32] : 0.f;
        }
        // ---- scores; the rows go to the value tile as they are split ----
        f32x16 acc[2], acc2[2];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                acc[t][r] = 0.f;
                acc2[t][r] = 0.f;
            }
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            float4 x0 = nrow[2 * q], x1 = nrow[2 * q + 1];
            if (FRB && q >= 2) {
                x1 = unpack_bf16x4(make_uint2(__float_as_uint(x0.z), __float_as_uint(x0.w)));
                x0 = unpack_bf16x4(make_uint2(__float_as_uint(x0.x), __float_as_uint(x0.y)));
            }
            *reinterpret_cast<float4*>(V + c32 * PITCH + 16 * q + 8 * hl) = x0;
            *reinterpret_cast<float4*>(V + c32 * PITCH + 16 * q + 8 * hl + 4) = x1;
            const BPlanes<P> ap = b3_split8<P>(x0, x1);
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                BPlanes<P> bp;
#pragma unroll
                for (int pl = 0; pl < P; ++pl) bp.p[pl] = W1[((q * NT + t) * P + pl) * 64 + lane];
                acc[t] = b3_mfma6<P>(ap, bp, acc[t]);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        fetch_row(tile + stride);       // (uses the index fetched one iteration ago)
        fetch_idx(tile + 2 * stride);
        __builtin_amdgcn_sched_barrier(0);
        wave_lds_sync();
        // ---- per point: value rows (LDS), softmax, (backward) dS, direct term, dW ----
#pragma unroll
        for (int pi = 0; pi < 2; ++pi) {
            float fv[2][8];
            const float* Vl = V + (ln.row0() * PITCH + c32);  // (the lane's first row and its column once: the rest are constants)
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int j = 0; j < 8; ++j) fv[t][j] = Vl[attg_acc_row(8 * pi + j) * PITCH + 32 * t];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                if constexpr (!BWD) {
                    const AttGSoftmax sm = attg_softmax(acc[t], pi, fv[t]);
                    if (hl == 0 && 16 * pi < nvalid) a.agg[(size_t)((row0 >> 4) + pi) * 64 + 32 * t + c32] = sm.agg;
                } else {
                    attg_softmax_bwd<false>(acc[t], acc2[t], pi, fv[t], gd[t][pi]);
                }
            }
            if constexpr (BWD) {
                BPlanes<P> fvp[2], dp[2];
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    fvp[t] = b3_split8<P>(fv[t]);
                    dp[t] = attg_tile_planes<P>(acc[t], pi);
                }
#pragma unroll
                for (int it = 0; it < 2; ++it)
#pragma unroll
                    for (int ct = 0; ct < 2; ++ct) acc3[it][ct] = b3_mfma6<P>(fvp[it], dp[ct], acc3[it][ct]);
            }
        }
        wave_lds_sync();  // (the value tile is rewritten by the next iteration)
        if constexpr (BWD) {
            // ---- dF = direct + dS . W^T: the transposed tile of dS (lane = row, registers = columns) is the row operand, register for register ----
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) {
                __builtin_amdgcn_sched_barrier(0);
                // (the planes of dS a second time rather than a transposed tile kept alive through the loop over the points: 16 registers
                //  for 44 VALU instructions)
                const f32x16 T = tr.transposed<P>(acc[ct]);
                const BPlanes<P> tp[2] = {attg_tile_planes<P>(T, 0), attg_tile_planes<P>(T, 1)};
#pragma unroll
                for (int u = 0; u < 2; ++u)
#pragma unroll
                    for (int it = 0; it < 2; ++it) {
                        BPlanes<P> bp;
#pragma unroll
                        for (int pl = 0; pl < P; ++pl) bp.p[pl] = W2[(((2 * ct + u) * NT + it) * P + pl) * 64 + lane];
                        acc2[it] = b3_mfma6<P>(tp[u], bp, acc2[it]);
                    }
            }
            // ---- stores.  Split form: tile 0 is the gathered half's gradient (plain rows for the gather-reduction, never accumulated),
            //      tile 1 the f_xyz half's -- with FRB both in the format of the f_xyz rows (ps_set_train_act_bf16: bfloat16) ----
#pragma unroll
            for (int it = 0; it < 2; ++it) {
                const bool left = split && it == 0;
                float* out = left ? a.dfl_rows : a.df;
                const int pitch = left ? a.ld_rows : a.lddf, col = split ? c32 : 32 * it + c32;
                const bool accum = split && !left && a.df_accum != 0;
                if (FRB && split) attg_store_df(reinterpret_cast<__bf16*>(out) + (size_t)row0 * pitch, col, pitch, nvalid, accum, acc2[it], ln);
                else attg_store_df(out + (size_t)row0 * pitch, col, pitch, nvalid, accum, acc2[it], ln);
            }
        }
    }
    if constexpr (BWD) {
        float* out = dw_part + (size_t)(blockIdx.x * WAVES + wave) * 4096 + (ln.row0() * 64 + c32);
#pragma unroll
        for (int it = 0; it < 2; ++it)
#pragma unroll
            for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                for (int r = 0; r < 16; ++r) out[(32 * it + attg_acc_row(r)) * 64 + 32 * ct] = acc3[it][ct][r];
    }
}

bool att64_gemm_fits(const Tuning& tn, const AttTrainArgs& a, bool backward)
{
    if (!tn.att64_gemm) return false;  // (A/B knob)
    auto al = [](const void* q, int ld) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0 && ld % 4 == 0; };
    if (!al(a.f, a.ld)) return false;
    if (a.fr_bf16 && (!a.fl || a.ld % 8 != 0 || !a.bf16)) return false;  // (bfloat16 rows: split form, 16-byte loads of eight values, bf16-MLP mode)
    if (a.fl) {
        if (!al(a.fl, a.ldl) || (reinterpret_cast<uintptr_t>(a.idx) & 15) != 0 || a.n_q <= 0) return false;
        if (backward && !a.dfl_rows) return false;  // (the float-atomic scatter form: attpool_train.hip)
    }
    return a.R > 0 && a.R * 16 < (1ll << 31);
}

template <int P, bool BWD, int WAVES, bool FRB>
static int launch_attg64_f(ps_context* c, const AttTrainArgs& a, const uint4* w1, const uint4* w2, float* dW)
{
    const size_t smem = (size_t)4 * 2 * P * 64 * 16 * (BWD ? 2 : 1) + sizeof(float) * WAVES * 32 * 68;
    auto kern = attg64_kernel<P, BWD, WAVES, FRB>;
    if (smem > 48 * 1024) PS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    const int per_cu = std::max(1, (int)(160 * 1024 / smem));
    const int64_t tiles = (a.R * 16 + 31) / 32;
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>((tiles + WAVES - 1) / WAVES, 256 * per_cu));
    float* part = nullptr;
    if (BWD) {
        PS_TRY(c->red_ws.reserve(sizeof(float) * (size_t)blocks * WAVES * 4096 + 256));
        part = c->red_ws.as<float>();
    }
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(WAVES * 64), smem, c->stream, a, w1, w2, part);
    if (BWD) hipLaunchKernelGGL(reduce_partials_kernel<float>, dim3(ceil_div(4096, 16)), dim3(256), 0, c->stream, static_cast<const float*>(part), blocks * WAVES, 4096, dW);
    PS_HIP(hipGetLastError());
    return PS_OK;
}

template <int P, bool BWD, int WAVES>
static int launch_attg64(ps_context* c, const AttTrainArgs& a, const uint4* w1, const uint4* w2, float* dW)
{
    if constexpr (P == 1) {  // (bfloat16 rows exist in the bf16-MLP mode only)
        if (a.fr_bf16) return launch_attg64_f<P, BWD, WAVES, true>(c, a, w1, w2, dW);
    }
    return launch_attg64_f<P, BWD, WAVES, false>(c, a, w1, w2, dW);
}

int att64_gemm(ps_context* c, AttTrainArgs a, bool backward, float* dW)
{
    const uint4 *w1 = nullptr, *w2 = nullptr;
    PS_TRY(attg_planes(c, a.w, 64, false, &w1));
    if (backward) PS_TRY(attg_planes(c, a.w, 64, true, &w2));
    // forward: twelve waves per workgroup (weights 24 KB + 8.5 KB of value tile per wave: three waves per SIMD); backward: 160 accumulator
    // registers + the prefetched rows -- four waves per workgroup or eight (two per SIMD; when this choice was measured, with 23 / 57
    // registers of scratch at P = 1 / 3 -- since attpool_gemm_kit.h's stores only bfloat16 rows spill, 25).  Measured on MI355X, 8 x 45 000
    // points (profiles/tools/exp_att64.py): fp32 1.349 ms with four, 1.443 with eight; bf16 0.858 with four, 0.713 with eight
    // (attpool_train.hip's kernels: 1.720 / 1.123).  PS_ATT64_OCC = 1 | 2 overrides.
    const int occ_env = c->tune.att64_occ;
    if (c->train_bf16) {
        if (!backward) return launch_attg64<1, false, 12>(c, a, w1, w2, dW);
        return occ_env == 1 ? launch_attg64<1, true, 4>(c, a, w1, w2, dW) : launch_attg64<1, true, 8>(c, a, w1, w2, dW);
    }
    if (!backward) return launch_attg64<3, false, 12>(c, a, w1, w2, dW);
    return occ_env == 2 ? launch_attg64<3, true, 8>(c, a, w1, w2, dW) : launch_attg64<3, true, 4>(c, a, w1, w2, dW);
}

// one array of rows an op reads or writes with 16-byte accesses: `width` columns at pitch ld
static bool attg_rows_ok(const void* p, int64_t ld, int64_t width) { return ld % 4 == 0 && ld >= width && (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
static bool attg_ok(int64_t K, int64_t d, const void* f, int64_t ld) { return ps_op_att_pool_gemm_supported(K, d) != 0 && attg_rows_ok(f, ld, d); }
/* split-source forms: F = [fl[idx] | fr] is never materialised (include/pointseg_train_ops.h); the split-source kernels end at d = 256 */
static bool attg_split_ok(const float* fl, int64_t ldl, const int32_t* idx, int64_t B, int64_t n_src, int64_t n_q, const float* fr, int64_t ldr, int64_t K, int64_t d)
{
    return ps_op_att_pool_gemm_supported(K, d) != 0 && d <= 256 && fl && idx && fr && attg_rows_ok(fl, ldl, d / 2) && attg_rows_ok(fr, ldr, d / 2) &&
           (reinterpret_cast<uintptr_t>(idx) & 15) == 0 && B >= 0 && n_src > 0 && n_q > 0 && n_src * ldl < (1ll << 31) && B * n_q * K < (1ll << 31);
}

// What an entry point was given.  The four fill the fields they have (the rest stay zero); attg_run checks them, fills AttGArgs and launches.
struct AttGCall {
    const char* null_msg;  // materialised forms: a NULL pointer has a message of its own
    const char* rule_msg;  // every other refusal: format over (K, d, ld, lddf, ldds)
    bool bwd, split;
    const float* f; int64_t ld;                                                    // fset, or fr of the split form
    const float* fl; int64_t ldl; const int32_t* idx; int64_t B, n_src, n_q;       // split form
    const float *wfc, *dagg; float* agg;
    float* df; int64_t lddf; int accumulate;                                       // dfset, or dfr of the split form
    float* dfl_rows; int64_t ld_rows;
    float* ds; int64_t ldds;
    int64_t R, K, d;
};

static int attg_run(ps_context* c, const AttGCall& q)
{
    const int64_t w = q.split ? q.d / 2 : q.d;  // columns of f / df
    const bool ptrs = c && q.wfc && (q.split || q.f) && (q.bwd ? q.dagg && q.df && q.ds && (!q.split || q.dfl_rows) : q.agg != nullptr);
    if (q.null_msg) PS_CHECK(ptrs, "%s", q.null_msg);
    bool ok = ptrs && (q.split ? attg_split_ok(q.fl, q.ldl, q.idx, q.B, q.n_src, q.n_q, q.f, q.ld, q.K, q.d) : attg_ok(q.K, q.d, q.f, q.ld) && q.R * q.K < (1ll << 31));
    // (dfset / dfl_rows / dscores leave in 16-byte stores: their bases and pitches are checked like the inputs')
    if (q.bwd) ok = ok && attg_rows_ok(q.df, q.lddf, w) && (!q.split || attg_rows_ok(q.dfl_rows, q.ld_rows, w)) && attg_ok(q.K, q.d, q.ds, q.ldds);
    PS_CHECK(ok, q.rule_msg, (long long)q.K, (long long)q.d, (long long)q.ld, (long long)q.lddf, (long long)q.ldds);
    if (q.R <= 0) return PS_OK;
    PS_HIP(hipSetDevice(c->device));
    Stage st(c, q.bwd ? "train_att_gemm_bwd" : "train_att_gemm_fwd", q.bwd ? 3 : 2);
    AttGArgs a = {};
    a.f = q.f; a.ld = (int)q.ld; a.fl = q.fl; a.ldl = (int)q.ldl; a.idx = q.idx; a.n_src = q.n_src; a.n_q = q.n_q;
    a.agg = q.agg; a.dagg = q.dagg; a.df = q.df; a.lddf = (int)q.lddf; a.df_accum = q.accumulate ? 1 : 0; a.dfl_rows = q.dfl_rows; a.ld_rows = (int)q.ld_rows;
    a.ds = q.ds; a.ldds = (int)q.ldds; a.rows = q.R * q.K; a.points = q.R;
    if (q.split && !q.bwd) {
        a.f_bf16 = c->train_act_bf16 && c->train_bf16 ? 1 : 0;  // (fr as bfloat16 rows, ldr in elements: ps_set_train_act_bf16; d = 128)
        PS_CHECK(!a.f_bf16 || (q.d == 128 && q.ld % 8 == 0), "ps_op_att_pool_gemm_fwd_split: bfloat16 rows: d = 128, ldr %% 8 == 0");
    }
    PS_TRY(attg_planes(c, q.wfc, q.d, false, &a.w1));
    if (q.bwd) PS_TRY(attg_planes(c, q.wfc, q.d, true, &a.w2));
    return launch_attg(c, a, q.d, q.bwd);
}

}  // namespace ps

using namespace ps;

extern "C" int ps_op_att_pool_gemm_supported(int64_t K, int64_t d) { return K == 16 && (d == 128 || d == 256 || d == 512) ? 1 : 0; }

extern "C" int ps_op_att_pool_gemm_fwd(ps_context* c, const float* fset, int64_t ld, const float* wfc, int64_t R, int64_t K, int64_t d, float* agg)
{
    AttGCall q = {};
    q.null_msg = "ps_op_att_pool_gemm_fwd: NULL argument";
    q.rule_msg = "ps_op_att_pool_gemm_fwd: K = 16, d in {128, 256, 512}, rows 16-byte aligned (got K %lld, d %lld, ld %lld)";
    q.f = fset; q.ld = ld; q.wfc = wfc; q.agg = agg; q.R = R; q.K = K; q.d = d;
    return attg_run(c, q);
}

extern "C" int ps_op_att_pool_gemm_bwd(ps_context* c, const float* fset, int64_t ld, const float* wfc, const float* dagg, int64_t R, int64_t K, int64_t d,
                                       float* dfset, int64_t lddf, int accumulate, float* dscores, int64_t ldds)
{
    AttGCall q = {};  // (d = 512 runs as two launches over halves of the dF columns)
    q.null_msg = "ps_op_att_pool_gemm_bwd: NULL argument";
    q.rule_msg = "ps_op_att_pool_gemm_bwd: K = 16, d in {128, 256, 512}, rows of fset / dfset / dscores 16-byte aligned with pitches %% 4 == 0 (got K %lld, d %lld, ld %lld, lddf %lld, ldds %lld)";
    q.bwd = true; q.R = R; q.K = K; q.d = d;
    q.f = fset; q.ld = ld; q.wfc = wfc; q.dagg = dagg; q.df = dfset; q.lddf = lddf; q.accumulate = accumulate; q.ds = dscores; q.ldds = ldds;
    return attg_run(c, q);
}

extern "C" int ps_op_att_pool_gemm_fwd_split(ps_context* c, const float* fl, int64_t ldl, const int32_t* idx, int64_t B, int64_t n_src, int64_t n_q,
                                             const float* fr, int64_t ldr, const float* wfc, int64_t K, int64_t d, float* agg)
{
    AttGCall q = {};
    q.rule_msg = "ps_op_att_pool_gemm_fwd_split: K = 16, d in {128, 256}, rows and the index table 16-byte aligned (got K %lld, d %lld)";
    q.split = true; q.R = B * n_q; q.K = K; q.d = d;
    q.fl = fl; q.ldl = ldl; q.idx = idx; q.B = B; q.n_src = n_src; q.n_q = n_q; q.f = fr; q.ld = ldr; q.wfc = wfc; q.agg = agg;
    return attg_run(c, q);
}

extern "C" int ps_op_att_pool_gemm_bwd_split(ps_context* c, const float* fl, int64_t ldl, const int32_t* idx, int64_t B, int64_t n_src, int64_t n_q,
                                             const float* fr, int64_t ldr, const float* wfc, const float* dagg, int64_t K, int64_t d, float* dfl_rows,
                                             int64_t ld_rows, float* dfr, int64_t lddr, int accumulate, float* dscores, int64_t ldds)
{
    AttGCall q = {};
    q.rule_msg = "ps_op_att_pool_gemm_bwd_split: K = 16, d in {128, 256}, every row array (inputs, dfl_rows, dfr, dscores) and the index table 16-byte aligned with pitches %% 4 == 0 (got K %lld, d %lld)";
    q.bwd = q.split = true; q.R = B * n_q; q.K = K; q.d = d;
    q.fl = fl; q.ldl = ldl; q.idx = idx; q.B = B; q.n_src = n_src; q.n_q = n_q; q.f = fr; q.ld = ldr; q.wfc = wfc; q.dagg = dagg;
    q.dfl_rows = dfl_rows; q.ld_rows = ld_rows; q.df = dfr; q.lddf = lddr; q.accumulate = accumulate; q.ds = dscores; q.ldds = ldds;
    return attg_run(c, q);
}
