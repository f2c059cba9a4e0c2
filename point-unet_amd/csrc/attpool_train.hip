// attpool_train.hip -- attentive pooling of the TRAINING step, forward and backward, fused per point.
//
//   att_pooling (PointSegment/RandLANet.py:388-398):   s = F . Wfc   (F = [N*K, d] neighbour set, no bias)
//                                                      p = softmax over the K rows of a point, per channel
//                                                      agg[n, c] = sum_k p[n,k,c] * F[n,k,c]
//
// The op-by-op formulation writes s and p ([N*K, d] each: 1.5 GB at levels 0 and 1 of a batch of 8 x 180 000 points), reads them
// back in the backward together with dscores / dF, and runs the three d x d GEMMs (scores, input gradient, weight gradient) as
// separate passes over those tensors.  Here a wave takes one point (its K x d tile of F goes to LDS once):
//   forward   scores on the MFMA from the LDS tile, softmax with wave shuffles, weighted sum -> only agg is written
//   backward  scores and softmax RECOMPUTED from the tile; with a = agg (recomputed), g = dagg:
//                 dS[k,c] = p[k,c] g[c] (F[k,c] - a[c])
//                 dF      = p . g  +  dS . Wfc^T          (second MFMA product, seeded with the direct term)
//                 dWfc   += F^T . dS                       (third MFMA product, accumulated over the wave's points in registers)
//             -> reads F and dagg, writes dF; per-workgroup dWfc partials go to a workspace that a second tiny kernel sums in
//                a fixed order (deterministic, no float atomics)
// Traffic per attention stage: forward 1 read of F (was: F read twice, s written + read, p written); backward 1 read of F + 1 write
// of dF (was ~8 passes).  The d x d weights (and their transpose) live in LDS; compiled for d = 16, 32, 64 (encoder levels 0 and 1,
// where the [N*K, d] tensors are large) and, in the bf16 mode, d = 128; wider levels keep the op-by-op path, whose tensors are small there.
// Two matrix pipes (attpool_train_kit.h): fp32 operands on the fp32 MFMA, and -- Trainer(mlp_dtype="bf16") -- operands rounded to bfloat16
// on the bf16 MFMA with fp32 accumulation.  Every a.bf16 call goes to the bf16 pipe: the fp32 kernels never round (the run-time rounding
// switch they once carried cost a select chain per element in an issue-bound loop).
#include "attpool_train_kit.h"
#include "reduce_partials.h"

#include <map>
#include <mutex>

namespace ps {

template <class Pipe, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void att_train_fwd_kernel(AttTrainArgs a)
{
    constexpr int D = Pipe::D, KN = Pipe::KN, NT = Pipe::NT;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, g = lane >> 4, c16 = lane & 15;  // (wave: an SGPR -- the point walk and every row base derived from it stay on the scalar unit)
    const Pipe P(smem, false, wave);
    P.template stage_weights<WAVES * 64>(a.w);
    __syncthreads();
    PointWalk w((int)(blockIdx.x * WAVES + wave), (int)(gridDim.x * WAVES), (int)a.n_q);
    TileRegs<D, KN, 64> regs;
    if (w.p < a.R) regs.fetch(a, w, lane);
    for (; w.p < a.R; w = w.next()) {
        const int64_t p = w.p;
        regs.expand(a, lane), P.commit(regs, lane);
        wave_lds_sync();
        const PointWalk wn = w.next();
        if (wn.p < a.R) regs.fetch(a, wn, lane);  // the next point's tile travels while this one is worked on
#pragma unroll
        for (int ct = 0; ct < NT; ++ct) {  // (tile by tile here: the all-tiles form measured 3 % slower in the forward)
            const AttSoftmax t = att_softmax_tile(P, P.score_tile(ct, lane), ct, g, c16);
            if (g == 0) a.agg[(size_t)p * D + ct * 16 + c16] = t.agg;
        }
        wave_lds_sync();
    }
}

// The one-wave-per-point backward kernels, per point: [tile and dagg of the NEXT point requested] -> scores / softmax / dS -> the two
// products, dF staged in the value tile -> staged rows to registers -> next tile committed -> stores issued.  Loads and stores so have a
// whole point's work to complete in.  The order of the products is each pipe's measured choice (and fixes the bits of dWfc).  This is the
// common end of a point: the staged dF rows leave, the prefetched tile lands.
template <class Pipe>
__device__ __forceinline__ void att_bwd_point_end(const Pipe& P, const AttTrainArgs& a, TileRegs<Pipe::D, Pipe::KN, 64>& regs, int64_t p, bool more, int lane)
{
    wave_lds_sync();
    RowStore<Pipe::D, Pipe::KN, Pipe::PA, 64> out;
    if (a.vec_store) {
        out.take(P.A, lane);
        wave_lds_sync();
    }
    if (more) regs.expand(a, lane), P.commit(regs, lane);
    if (a.vec_store) out.put(a, p, lane);
    wave_lds_sync();
}

template <int D, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void att_train_bwd_kernel(AttTrainArgs a)
{
    using Pipe = AttF32Pipe<D>;
    constexpr int KN = Pipe::KN, NT = Pipe::NT;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, g = lane >> 4, c16 = lane & 15;  // (wave: an SGPR -- the point walk and every row base derived from it stay on the scalar unit)
    const Pipe P(smem, true, wave);
    P.template stage_weights<WAVES * 64>(a.w);
    __syncthreads();

    f32x4 dw[NT][NT] = {};  // this wave's share of dWfc: tile (ti, tj) = rows 16 ti.., columns 16 tj..
    PointWalk w((int)(blockIdx.x * WAVES + wave), (int)(gridDim.x * WAVES), (int)a.n_q);
    TileRegs<D, KN, 64> regs;
    float gnext[NT];
    if (w.p < a.R) {
        regs.fetch(a, w, lane);
        att_load_dagg<D>(a, w.p, 0, c16, gnext);
        regs.expand(a, lane), P.commit(regs, lane);
    }
    wave_lds_sync();
    for (; w.p < a.R; w = w.next()) {
        const int64_t p = w.p;
        const PointWalk wn = w.next();
        float gcur[NT];
#pragma unroll
        for (int ct = 0; ct < NT; ++ct) gcur[ct] = gnext[ct];
        if (wn.p < a.R) {
            regs.fetch(a, wn, lane);
            att_load_dagg<D>(a, wn.p, 0, c16, gnext);
        }
        f32x4 dfd[NT];  // direct term p * g of every column tile (seeds the second product)
        f32x4 sc_all[NT];
        P.score_tiles(lane, sc_all);
#pragma unroll
        for (int ct = 0; ct < NT; ++ct) dfd[ct] = att_ds_tile(P, att_softmax_tile(P, sc_all[ct], ct, g, c16), gcur[ct], ct, g, c16);
        wave_lds_sync();
        P.dw_accumulate(dw, 0, g, c16);
        if (a.vec_store) wave_lds_sync();  // the value tile is dead from here on: it stages dF for the 16-byte stores
        // dF = p . g + dS . Wfc^T  (tile by tile: the all-tiles form of the scores measured no better here)
#pragma unroll
        for (int tj = 0; tj < NT; ++tj) att_put_df(P, a, p, tj, g, c16, P.df_tile(tj, lane, dfd[tj]));
        att_bwd_point_end(P, a, regs, p, wn.p < a.R, lane);
    }
    att_reduce_dw<D, WAVES>(smem, dw, a.dw_part, wave, g, c16);
}

template <int D, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void att_train_bwd_bf16_kernel(AttTrainArgs a)
{
    using Pipe = AttBf16Pipe<D>;
    constexpr int KN = Pipe::KN, NT = Pipe::NT;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, g = lane >> 4, c16 = lane & 15;  // (wave: an SGPR -- the point walk and every row base derived from it stay on the scalar unit)
    const Pipe P(smem, true, wave);
    P.template stage_weights<WAVES * 64>(a.w);
    __syncthreads();

    f32x4 dw[NT][NT] = {};  // this wave's share of dWfc: tile (ti, tj) = rows 16 ti.., columns 16 tj..
    PointWalk w((int)(blockIdx.x * WAVES + wave), (int)(gridDim.x * WAVES), (int)a.n_q);
    TileRegs<D, KN, 64> regs;
    float gnext[NT];
    if (w.p < a.R) {
        regs.fetch(a, w, lane);
        att_load_dagg<D>(a, w.p, 0, c16, gnext);
        regs.expand(a, lane), P.commit(regs, lane);
    }
    wave_lds_sync();
    for (; w.p < a.R; w = w.next()) {
        const int64_t p = w.p;
        const PointWalk wn = w.next();
        float gcur[NT];
#pragma unroll
        for (int ct = 0; ct < NT; ++ct) gcur[ct] = gnext[ct];
        if (wn.p < a.R) {
            regs.fetch(a, wn, lane);
            att_load_dagg<D>(a, wn.p, 0, c16, gnext);
        }
        f32x4 dfd[NT];  // direct term p * g of every column tile (seeds the second product)
#pragma unroll
        for (int ct = 0; ct < NT; ++ct) dfd[ct] = att_ds_tile(P, att_softmax_tile(P, P.score_tile(ct, lane), ct, g, c16), gcur[ct], ct, g, c16);
        wave_lds_sync();
        // dF = p . g + dS . Wfc^T  (the fp32 value tile is dead after the softmax loop: it stages dF for the 16-byte stores)
#pragma unroll
        for (int tj = 0; tj < NT; ++tj) att_put_df(P, a, p, tj, g, c16, P.df_tile(tj, lane, dfd[tj]));
        P.dw_accumulate(dw, 0, g, c16);
        att_bwd_point_end(P, a, regs, p, wn.p < a.R, lane);
    }
    if constexpr (att_wave_partials(D, WAVES)) {
        // d = 128: WAVES x D x D floats do not fit LDS -- every WAVE stores its own partial (the fixed-order reduction behind this kernel
        // simply sees WAVES times as many rows)
        att_store_dw<D, NT>(a.dw_part + ((size_t)blockIdx.x * WAVES + wave) * D * D, dw, 0, g, c16);
    } else {
        att_reduce_dw<D, WAVES>(smem, dw, a.dw_part, wave, g, c16);
    }
}

// ---- column-split backward (bf16 mode, d = 128): FOUR waves share one point ---------------------------------------------------------------
// At d = 128 the kernel above holds 64 x 4 dWfc accumulators per wave (464 registers: one wave per SIMD) and 17.5 KB of tiles per wave next
// to 74 KB of weights (four waves per CU): every point is one long serial chain -- fetch, scores, softmax, dS, two products, stores -- with
// nothing to hide its latencies.  Here the four waves of a GROUP work on the same point and split the column tiles of every phase: a wave
// computes the scores / softmax / dS of its D/64 column tiles (a 16 x 16 tile holds all K rows of its channels: the softmax stays inside
// the wave), accumulates the matching columns of dWfc (64 x 4 / 4 accumulators), and -- once all of dS is in LDS -- its column tiles of
// dF = p g + dS . Wfc^T.  The group shares ONE set of tiles (its 256 lanes fetch, commit and store them together), so a workgroup of GROUPS
// groups fits 4 GROUPS waves, each a quarter as long per point.  Workgroup barriers separate the phases (all groups take the same number of
// iterations; a group past the end idles through them).  Row outputs only (df / dfl_rows as 16-byte stores): the deterministic step's form.
template <int D, int GROUPS>
__global__ __launch_bounds__(GROUPS * 256) void att_train_bwd_bf16_cs_kernel(AttTrainArgs a)
{
    using Pipe = AttBf16Pipe<D>;
    static_assert(D % 64 == 0, "column tiles split over four waves");
    constexpr int KN = Pipe::KN, NT = Pipe::NT, NTW = NT / 4;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, g = lane >> 4, c16 = lane & 15;  // (wave: an SGPR -- the point walk and every row base derived from it stay on the scalar unit)
    const int grp = wave >> 2, wj = wave & 3, glane = (wj << 6) | lane, c0 = wj * NTW;  // (c0: this wave's first column tile)
    const Pipe P(smem, true, grp);
    P.template stage_weights<GROUPS * 256>(a.w);

    f32x4 dw[NT][NTW] = {};  // rows 16 ti.., this wave's column tiles c0 + t
    const int stride = (int)gridDim.x * GROUPS;
    const int first_of_block = (int)blockIdx.x * GROUPS;
    const int iters = first_of_block < a.R ? (int)((a.R - first_of_block + stride - 1) / stride) : 0;  // of the block's FIRST group: the most
    PointWalk w(first_of_block + grp, stride, (int)a.n_q);
    TileRegs<D, KN, 256> regs;
    float gnext[NTW];
    if (w.p < a.R) {
        regs.fetch(a, w, glane);
        att_load_dagg<D>(a, w.p, c0, c16, gnext);
        regs.expand(a, glane), P.commit(regs, glane);
    }
    __syncthreads();  // weights and the first tiles
    for (int it = 0; it < iters; ++it, w = w.next()) {
        const bool live = w.p < a.R;
        const int64_t p = w.p;
        const PointWalk wn = w.next();
        const bool more = wn.p < a.R;
        float gcur[NTW];
#pragma unroll
        for (int t = 0; t < NTW; ++t) gcur[t] = gnext[t];
        if (more) {
            regs.fetch(a, wn, glane);
            att_load_dagg<D>(a, wn.p, c0, c16, gnext);
        }
        f32x4 dfd[NTW];
        if (live) {
#pragma unroll
            for (int t = 0; t < NTW; ++t) dfd[t] = att_ds_tile(P, att_softmax_tile(P, P.score_tile(c0 + t, lane), c0 + t, g, c16), gcur[t], c0 + t, g, c16);
            wave_lds_sync();  // (this wave's own dS columns)
            P.dw_accumulate(dw, c0, g, c16);
        }
        __syncthreads();  // all of dS is in LDS
        if (live) {
#pragma unroll
            for (int t = 0; t < NTW; ++t) att_stage_df(P, c0 + t, g, c16, P.df_tile(c0 + t, lane, dfd[t]));  // (the value tile is dead: it stages dF)
        }
        __syncthreads();  // dF staged, dS read by everyone
        RowStore<D, KN, Pipe::PA, 256> out;
        if (live) out.take(P.A, glane);
        __syncthreads();  // the staged tile is in registers: the next point's tile may land
        if (more) regs.expand(a, glane), P.commit(regs, glane);
        if (live) out.put(a, p, glane);
        __syncthreads();  // the next tile is visible
    }
    // the group's dWfc partial: its four waves hold disjoint column tiles
    att_store_dw<D, NTW>(a.dw_part + ((size_t)blockIdx.x * GROUPS + grp) * D * D, dw, c0, g, c16);
}

// Workgroups per launch: every workgroup walks the points with the same stride, so a grid that is not a multiple of what the chip holds at
// once ends with a round at partial occupancy (the d = 16 backward: 77 VGPRs allow three 8-wave workgroups per CU where the LDS footprint
// alone allows four -- 1024 workgroups ran as 768 + 256, the second round as long as the first).  Ask the runtime what fits.
static int att_resident_blocks(const void* kern, int threads, size_t smem, int lds_guess)
{
    static std::mutex mu;
    static std::map<std::pair<const void*, size_t>, int> cache;  // (asked once per kernel and LDS size)
    std::lock_guard<std::mutex> lock(mu);
    auto it = cache.find({kern, smem});
    if (it != cache.end()) return it->second;
    int occ = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kern, threads, smem) != hipSuccess || occ < 1) {
        (void)hipGetLastError();
        occ = lds_guess;
    }
    cache[{kern, smem}] = occ;
    return occ;
}

// One launch: the LDS attribute, what the chip holds at once, the grid -- min(ceil(R / points_per_block), 256 occ) -- and, where the kernel
// leaves dw_parts_per_block > 0 partials of D x D per workgroup, their workspace and the fixed-order sum into dW behind the kernel.
static int att_launch(ps_context* c, AttTrainArgs a, void (*kern)(AttTrainArgs), int threads, size_t smem, int points_per_block, int dw_parts_per_block,
                      int dd, float* dW)
{
    PS_CHECK(smem <= 160 * 1024, "att_pool_train: %zu bytes of LDS needed", smem);
    const int per_cu = std::max(1, std::min(4, (int)(160 * 1024 / smem)));
    if (smem > 48 * 1024) PS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    const int occ = std::min(per_cu, att_resident_blocks(reinterpret_cast<const void*>(kern), threads, smem, per_cu));
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>((a.R + points_per_block - 1) / points_per_block, 256 * occ));
    const int parts = blocks * dw_parts_per_block;
    if (parts) {
        PS_TRY(c->red_ws.reserve(sizeof(float) * (size_t)parts * dd + 256));
        a.dw_part = c->red_ws.as<float>();
    }
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(threads), smem, c->stream, a);
    if (parts) hipLaunchKernelGGL(reduce_partials_kernel<float>, dim3(ceil_div(dd, 16)), dim3(256), 0, c->stream, static_cast<const float*>(a.dw_part), parts, dd, dW);
    PS_HIP(hipGetLastError());
    return PS_OK;
}

template <int D>
static int launch_att_train(ps_context* c, AttTrainArgs a, bool backward, float* dW)
{
    // d = 128 exists on the bf16 matrix pipe only (both weight orientations as bfloat16: 74 KB; in fp32 they are 147 KB): four waves per
    // workgroup in the backward (17.5 KB of tiles per wave, the 64 x 4 dWfc accumulators in AGPRs: one wave per SIMD), eight in the forward
    constexpr int WAVES = 8, WAVES_B = D == 128 ? 4 : 8;  // (d = 64 with twelve waves: 168 VGPRs, 34 spilled, 1.85 against 1.12 ms)
    if (backward) {
        auto al = [](const void* q, int ld) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0 && ld % 4 == 0; };
        const bool rows_out = !a.fl || a.dfl_rows;  // (the atomic scatter form keeps its per-element path)
        a.vec_store = rows_out && al(a.df, a.lddf) && (!a.fl || al(a.dfl_rows, a.ld_rows)) ? 1 : 0;
        PS_CHECK(!a.fr_bf16 || a.vec_store || a.bf16, "att_pool_train backward: bfloat16 rows (ps_set_train_act_bf16) belong to the bf16-MLP mode");
    }
    if constexpr (D == 64) {
        // level 1: the 32x32x16 bf16 matrix pipe (exact three-way splits in fp32 mode), weights resident in LDS, dWfc in registers
        // (attpool_gemm.hip: 0.63 -> 0.3 ms forward, 1.71 -> 0.9 ms backward per pooling of 5.76 M rows)
        if (att64_gemm_fits(c->tune, a, backward)) return att64_gemm(c, a, backward, dW);
    }
    if (a.bf16) {  // the bf16-MLP mode: operands kept as bfloat16 in LDS, products on the bf16 matrix pipe
        using P = AttBf16Pipe<D>;
        if (!backward) return att_launch(c, a, att_train_fwd_kernel<P, WAVES>, WAVES * 64, att_lds_bytes<P>(false, WAVES, 0), WAVES, 0, D * D, nullptr);
        if constexpr (D == 128) {
            // four waves per point (att_train_bwd_bf16_cs_kernel): three groups per workgroup share the 74 KB of weights: 897 us against
            // 1 192 us for the one-wave-per-point kernel.  (d = 64, four groups: 1 334 us against 1 100 us -- the barriers of a sixteen-wave
            // workgroup cost more than its shorter chains gain: not used there.)
            constexpr int GROUPS = 3;
            if (a.vec_store && !c->tune.att_no_split)
                return att_launch(c, a, att_train_bwd_bf16_cs_kernel<D, GROUPS>, GROUPS * 256, att_lds_bytes<P>(true, GROUPS, 0), GROUPS, GROUPS, D * D, dW);
        }
        constexpr bool per_wave = att_wave_partials(D, WAVES_B);
        return att_launch(c, a, att_train_bwd_bf16_kernel<D, WAVES_B>, WAVES_B * 64, att_lds_bytes<P>(true, WAVES_B, per_wave ? 0 : WAVES_B), WAVES_B,
                          per_wave ? WAVES_B : 1, D * D, dW);
    }
    if constexpr (D == 128) {
        set_error("att_pool_train: d = 128 is compiled for the bf16-MLP mode only (ps_set_train_gemm_bf16)");
        return PS_EINVAL;
    } else {
        using P = AttF32Pipe<D>;
        if (!backward) return att_launch(c, a, att_train_fwd_kernel<P, WAVES>, WAVES * 64, att_lds_bytes<P>(false, WAVES, 0), WAVES, 0, D * D, nullptr);
        return att_launch(c, a, att_train_bwd_kernel<D, WAVES>, WAVES * 64, att_lds_bytes<P>(true, WAVES, WAVES), WAVES, 1, D * D, dW);
    }
}

static int att_train_dispatch(ps_context* c, const AttTrainArgs& a, int64_t d, bool backward, float* dW)
{
    switch (d) {
        case 16: return launch_att_train<16>(c, a, backward, dW);
        case 32: return launch_att_train<32>(c, a, backward, dW);
        case 64: return launch_att_train<64>(c, a, backward, dW);
        default: return launch_att_train<128>(c, a, backward, dW);
    }
}

static bool att_train_ok(int64_t K, int64_t d, int64_t ld, const void* f)
{
    return K == 16 && (d == 16 || d == 32 || d == 64 || d == 128) && ld % 4 == 0 && (reinterpret_cast<uintptr_t>(f) & 15) == 0;
}

// both split-source backward entries: the gathered half's gradient scatter-added into dfl (dfl_rows == nullptr), or written as rows;
// df_accum: dfr += instead of dfr = (common.h)
int att_bwd_split_impl(ps_context* c, const float* fl, int64_t ldl, const int32_t* idx, int64_t B, int64_t n_src, int64_t n_q, const float* fr,
                       int64_t ldr, const float* wfc, const float* dagg, int64_t K, int64_t d, float* dfl, int64_t lddl, float* dfr, int64_t lddr,
                       float* dwfc, float* dfl_rows, int64_t ld_rows, bool df_accum)
{
    PS_CHECK(c && fl && idx && fr && wfc && dagg && dfl && dfr && dwfc, "ps_op_att_pool_train_bwd_split: NULL argument");
    PS_CHECK(att_train_ok(K, d, ldr, fr) && ldl % 4 == 0 && (reinterpret_cast<uintptr_t>(fl) & 15) == 0 && n_src * ldl < (1ll << 31) && lddl >= d / 2 && lddr >= d / 2 && n_src > 0,
             "ps_op_att_pool_train_bwd_split: K = 16, d in {16, 32, 64}, rows 16-byte aligned");
    PS_HIP(hipSetDevice(c->device));
    const int64_t R = B * n_q;
    if (R <= 0) {
        PS_HIP(hipMemsetAsync(dwfc, 0, sizeof(float) * d * d, c->stream));
        return PS_OK;
    }
    Stage st(c, "train_att_fused_bwd", 2);
    AttTrainArgs a = {};
    a.f = fr; a.ld = (int)ldr; a.fl = fl; a.ldl = (int)ldl; a.idx = idx; a.n_src = n_src; a.n_q = n_q;
    a.w = wfc; a.dagg = dagg; a.df = dfr; a.lddf = (int)lddr; a.dfl = dfl; a.lddl = (int)lddl; a.R = R; a.bf16 = c->train_bf16 ? 1 : 0;
    a.dfl_rows = dfl_rows; a.ld_rows = (int)ld_rows; a.df_accum = df_accum ? 1 : 0;
    a.fr_bf16 = c->train_act_bf16 && c->train_bf16 ? 1 : 0;  // (fr as bfloat16 rows: ps_set_train_act_bf16)
    return att_train_dispatch(c, a, d, true, dwfc);
}

}  // namespace ps

using namespace ps;

extern "C" int ps_op_att_pool_train_supported(int64_t K, int64_t d) { return K == 16 && (d == 16 || d == 32 || d == 64) ? 1 : 0; }
extern "C" int ps_op_att_pool_train_supported_ex(int64_t K, int64_t d, int bf16_mode)
{
    return K == 16 && (d == 16 || d == 32 || d == 64 || (d == 128 && bf16_mode)) ? 1 : 0;
}

extern "C" int ps_op_att_pool_train_fwd(ps_context* c, const float* fset, int64_t ld, const float* wfc, int64_t R, int64_t K, int64_t d, float* agg)
{
    PS_CHECK(c && fset && wfc && agg, "ps_op_att_pool_train_fwd: NULL argument");
    PS_CHECK(att_train_ok(K, d, ld, fset), "ps_op_att_pool_train_fwd: K = 16, d in {16, 32, 64}, rows 16-byte aligned (got K %lld, d %lld, ld %lld)",
             (long long)K, (long long)d, (long long)ld);
    if (R <= 0) return PS_OK;
    PS_HIP(hipSetDevice(c->device));
    Stage st(c, "train_att_fused_fwd", 1);
    AttTrainArgs a = {};
    a.f = fset; a.w = wfc; a.agg = agg; a.R = R; a.ld = (int)ld; a.bf16 = c->train_bf16 ? 1 : 0;
    return att_train_dispatch(c, a, d, false, nullptr);
}

extern "C" int ps_op_att_pool_train_bwd(ps_context* c, const float* fset, int64_t ld, const float* wfc, const float* dagg, int64_t R, int64_t K, int64_t d,
                                        float* dfset, int64_t lddf, float* dwfc)
{
    PS_CHECK(c && fset && wfc && dagg && dfset && dwfc, "ps_op_att_pool_train_bwd: NULL argument");
    PS_CHECK(att_train_ok(K, d, ld, fset) && lddf >= d, "ps_op_att_pool_train_bwd: K = 16, d in {16, 32, 64}, rows 16-byte aligned");
    PS_HIP(hipSetDevice(c->device));
    if (R <= 0) {
        PS_HIP(hipMemsetAsync(dwfc, 0, sizeof(float) * d * d, c->stream));
        return PS_OK;
    }
    Stage st(c, "train_att_fused_bwd", 2);
    AttTrainArgs a = {};
    a.f = fset; a.w = wfc; a.dagg = dagg; a.df = dfset; a.R = R; a.ld = (int)ld; a.lddf = (int)lddf; a.bf16 = c->train_bf16 ? 1 : 0;
    return att_train_dispatch(c, a, d, true, dwfc);
}

/* split-source form: F = [fl[idx] | fr] is never materialised (see include/pointseg.h) */
extern "C" int ps_op_att_pool_train_fwd_split(ps_context* c, const float* fl, int64_t ldl, const int32_t* idx, int64_t B, int64_t n_src, int64_t n_q,
                                              const float* fr, int64_t ldr, const float* wfc, int64_t K, int64_t d, float* agg)
{
    PS_CHECK(c && fl && idx && fr && wfc && agg, "ps_op_att_pool_train_fwd_split: NULL argument");
    PS_CHECK(att_train_ok(K, d, ldr, fr) && ldl % 4 == 0 && (reinterpret_cast<uintptr_t>(fl) & 15) == 0 && n_src * ldl < (1ll << 31) && B >= 0 && n_src > 0 && n_q >= 0,
             "ps_op_att_pool_train_fwd_split: K = 16, d in {16, 32, 64}, rows 16-byte aligned (got K %lld, d %lld)", (long long)K, (long long)d);
    const int64_t R = B * n_q;
    if (R <= 0) return PS_OK;
    PS_HIP(hipSetDevice(c->device));
    Stage st(c, "train_att_fused_fwd", 1);
    AttTrainArgs a = {};
    a.f = fr; a.ld = (int)ldr; a.fl = fl; a.ldl = (int)ldl; a.idx = idx; a.n_src = n_src; a.n_q = n_q;
    a.w = wfc; a.agg = agg; a.R = R; a.bf16 = c->train_bf16 ? 1 : 0;
    a.fr_bf16 = c->train_act_bf16 && c->train_bf16 ? 1 : 0;  // (fr as bfloat16 rows: ps_set_train_act_bf16)
    return att_train_dispatch(c, a, d, false, nullptr);
}

extern "C" int ps_op_att_pool_train_bwd_split(ps_context* c, const float* fl, int64_t ldl, const int32_t* idx, int64_t B, int64_t n_src, int64_t n_q,
                                              const float* fr, int64_t ldr, const float* wfc, const float* dagg, int64_t K, int64_t d, float* dfl,
                                              int64_t lddl, float* dfr, int64_t lddr, float* dwfc)
{
    PS_CHECK(dfl, "ps_op_att_pool_train_bwd_split: NULL argument");
    return att_bwd_split_impl(c, fl, ldl, idx, B, n_src, n_q, fr, ldr, wfc, dagg, K, d, dfl, lddl, dfr, lddr, dwfc, nullptr, 0, false);
}

extern "C" int ps_op_att_pool_train_bwd_split_rows(ps_context* c, const float* fl, int64_t ldl, const int32_t* idx, int64_t B, int64_t n_src, int64_t n_q,
                                                   const float* fr, int64_t ldr, const float* wfc, const float* dagg, int64_t K, int64_t d,
                                                   float* dfl_rows, int64_t ld_rows, float* dfr, int64_t lddr, float* dwfc)
{
    PS_CHECK(dfl_rows && ld_rows >= d / 2, "ps_op_att_pool_train_bwd_split_rows: dfl_rows is NULL or its row stride below d/2");
    return att_bwd_split_impl(c, fl, ldl, idx, B, n_src, n_q, fr, ldr, wfc, dagg, K, d, dfl_rows, ld_rows, dfr, lddr, dwfc, dfl_rows, ld_rows, false);
}
