// attpool32.hip -- fused LocSE + neighbour gather + attentive pooling for d_out >= 64 on v_mfma_f32_32x32x2_f32.
//
// Same computation as attpool.hip (building_block / relative_pos_encoding / gather_neighbour / att_pooling,
// PointSegment/RandLANet.py:323-343, 377-401, up to att_pooling's trailing conv2d; scores in the pre-product form
// G[idx] + f_xyz . Wfc[d/2:, :]), re-tiled:
//   * one MFMA tile = 32 rows = the K neighbours of 32/K points (two points at K = 16, one at K = 32) x 32 channels.  Against
//     the 16x16x4 tiling that is half the MFMA instructions and half the operand fetches per FLOP, the two points of a tile
//     share every weight fragment, and a channel's K scores sit in 8 (16) registers of two lanes: the softmax reductions
//     are in-lane plus ONE v_permlane32_swap instead of two cross-lane steps.
//   * operands move 16 bytes per lane: the K axis of every product is taken in the order {8q + 4*half + t} (q = chunk of 8
//     input channels, half = lane >> 5, t = MFMA step within the chunk), so a lane's operand values of four consecutive
//     MFMAs are one ds_read_b128 of the activation tile and one 16-byte read of the weight image packed to match (pack_p32).
//   * the two small products (LocSE mlp1, LFA mlp2) are evaluated transposed (C[channel][row]): a lane's four consecutive
//     accumulator registers are four consecutive channels of its row and go to the LDS tile as one ds_write_b128.
//   * d <= 128 (levels 1-2: many points): every wave owns a tile, eight waves per workgroup, the level's three weight
//     matrices live in LDS (52 KB at d = 128) -- no weight traffic per point at all; LFA mlp2's output is held in registers
//     until the wave has consumed the mlp1 tile and then overwrites it in place (one tile per wave).
//     d >= 256 (levels 3-4: few points): the waves of a workgroup share one tile and split its output-column blocks; the
//     weights stream from L2 with 16-byte loads (a fragment serves two points).
// LDS tile pitch = H + 4 floats = 4 x odd: conflict-free for the b128 reads and writes above (MI355X_MICROARCH.md, LDS).
//
// Bound: fp32 MFMA.  Per point: (d/32) * (h/2) score MFMAs of 64 cycles per pair of points, e.g. d = 128: 128 + 64 (mlp2) + 10.
// The tile frame -- walk, geometry prefetch, neighbour-row offsets, bias seed, tile store, pooling of a score block -- is att32_tile.h's,
// one text shared with the split-bf16 kernels of attpool32b.hip, which are judged against this one.
#include "att32_tile.h"

namespace ps {

struct Att32Args : Att32ArgsT<float> {};  // w1: [H/32][5][64] image (pack_p32_locse); w2, wb: pack_p32 images

template <int D, int STAGE, int KN, int WAVES, bool SPLITN>
__global__ __launch_bounds__(WAVES * 64) void att32_kernel(Att32Args a)
{
    constexpr int H = D / 2, LDF = H + D, PITCH = H + 4, PPT = 32 / KN;
    constexpr int CBH = H / 32, CBD = D / 32, NQ = H / 8;
    constexpr int W1F = CBH * 5 * 64, W2F = STAGE == 2 ? H * H : 0, WBF = H * D;
    constexpr int TILE = 32 * PITCH;
    static_assert(H % 32 == 0 && (KN == 16 || KN == 32), "att32: d_out >= 64, K in {16, 32}");

    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int hl = lane >> 5, c32 = lane & 31;
    // LDS: [weights + biases (wave-per-tile form only)] [per tile owner: 32 neighbour rows | tile(s)]
    float* Ws = smem;
    constexpr int WTOT = SPLITN ? 0 : (W1F + W2F + WBF + 2 * H);
    float* own = smem + WTOT + (SPLITN ? 0 : wave) * (32 + TILE);
    int* NB = reinterpret_cast<int*>(own);
    float* T1 = own + 32;
    float* T2 = SPLITN && STAGE == 2 ? T1 + TILE : T1;
    const float *w1 = a.w1, *w2 = a.w2, *wb = a.wb, *b1 = a.b1, *b2 = a.b2;
    if constexpr (!SPLITN) {
        for (int i = threadIdx.x; i < W1F; i += WAVES * 64) Ws[i] = a.w1[i];
        for (int i = threadIdx.x; i < W2F / 4; i += WAVES * 64) reinterpret_cast<float4*>(Ws + W1F)[i] = reinterpret_cast<const float4*>(a.w2)[i];
        for (int i = threadIdx.x; i < WBF / 4; i += WAVES * 64) reinterpret_cast<float4*>(Ws + W1F + W2F)[i] = reinterpret_cast<const float4*>(a.wb)[i];
        for (int i = threadIdx.x; i < H; i += WAVES * 64) {
            Ws[W1F + W2F + WBF + i] = a.b1[i];
            Ws[W1F + W2F + WBF + H + i] = STAGE == 2 ? a.b2[i] : 0.f;
        }
        __syncthreads();
        w1 = Ws; w2 = Ws + W1F; wb = Ws + W1F + W2F; b1 = Ws + W1F + W2F + WBF; b2 = b1 + H;
    }
    constexpr int CBSTEP = SPLITN ? WAVES : 1;
    const int cb0 = SPLITN ? wave : 0;
    auto phase_sync = [&]() {
        if constexpr (SPLITN) __syncthreads();
        else wave_lds_sync();
    };

    constexpr int TPW = SPLITN ? 1 : WAVES;
    const int tiw = SPLITN ? 0 : wave;
#include "att32_tile_walk.h"
    for (int t0 = t_first; t0 < t_end; t0 += t_step) {
#include "att32_tile_row.h"
        // MFMA step s takes elements 2s (lanes 0-31) and 2s + 1 (lanes 32-63) of enc10
        float e[5];
        e[0] = hl ? enc[1] : enc[0]; e[1] = hl ? enc[3] : enc[2]; e[2] = hl ? enc[5] : enc[4]; e[3] = hl ? enc[7] : enc[6]; e[4] = hl ? enc[9] : enc[8];
        if (hl == 0 && (!SPLITN || wave == 0)) NB[c32] = nbr;
        gstage(0, t0 + t_step);

        // ---- LFA mlp1 (transposed: C[channel][row]): f_xyz1 = lrelu(enc10 . W1 + b1) -> T1 ----
#pragma unroll
        for (int cb = cb0; cb < CBH; cb += CBSTEP) {
            f32x16 acc;
            ATT32_BIAS_SEED(acc, b1, cb);
#pragma unroll
            for (int s = 0; s < 5; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w1[(cb * 5 + s) * 64 + lane], e[s], acc, 0, 0, 0);
            ATT32_STORE_BLOCK(T1 + c32 * PITCH, cb, leaky02, acc);
        }
        phase_sync();
        gstage(1, t0 + t_step);
        if constexpr (STAGE == 2) {
            // ---- LFA mlp2 (transposed): f_xyz2 = lrelu(f_xyz1 . W2 + b2) ----
            constexpr int NACC = SPLITN ? 1 : CBH;
            f32x16 acc2[NACC];
#pragma unroll
            for (int cb = cb0; cb < CBH; cb += CBSTEP) {
                f32x16& acc = acc2[SPLITN ? 0 : cb];
                ATT32_BIAS_SEED(acc, b2, cb);
                const float4* wq = reinterpret_cast<const float4*>(w2) + (size_t)cb * NQ * 64 + lane;
                const float* xr = T1 + c32 * PITCH + 4 * hl;
#pragma unroll 8
                for (int q = 0; q < NQ; ++q) {
                    const float4 aw = wq[(size_t)q * 64];
                    const float4 bx = *reinterpret_cast<const float4*>(xr + 8 * q);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(aw.x, bx.x, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(aw.y, bx.y, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(aw.z, bx.z, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(aw.w, bx.w, acc, 0, 0, 0);
                }
                if constexpr (SPLITN) { ATT32_STORE_BLOCK(T2 + c32 * PITCH, cb, leaky02, acc); }
            }
            if constexpr (!SPLITN) {
                wave_lds_sync();  // every read of the mlp1 tile precedes the writes below (DS operations of a wave execute in order)
#pragma unroll
                for (int cb = 0; cb < CBH; ++cb) { ATT32_STORE_BLOCK(T1 + c32 * PITCH, cb, leaky02, acc2[cb]); }
            }
            phase_sync();
        }
        const float* TX = T2;

        // ---- scores (C[row][channel]) = G[nbr] + f_xyz . Wfc[H:, :], softmax over the K rows of a point, weighted sum ----
        unsigned off[16];  // of this lane's column of the wave's first column block
        ATT32_ROW_OFFSETS(off, NB, LDF, (unsigned)(cb0 * 32 + c32) * 4u);
        const char* fgb = reinterpret_cast<const char*>(a.fg);
        // The gathers of column block i + 1 (G rows for the scores, f rows for the values) are issued before the MFMAs of block i
        // and consumed after them: their latency hides behind ~2 000 cycles of matrix work.  G is ADDED after the product
        // (instead of seeding the accumulator) for the same reason.
        constexpr int NCB = CBD / CBSTEP;
        f32x2 gq[2][8], v[2][8];
        auto gather = [&](int i, f32x2 (&gdst)[8], f32x2 (&vdst)[8]) {
            const int rel = i * CBSTEP * 32 * 4;  // compile-time (the loop below is fully unrolled)
#pragma unroll
            for (int r = 0; r < 16; ++r) gdst[r >> 1][r & 1] = *reinterpret_cast<const float*>(fgb + off[r] + (rel + H * 4));
            if ((cb0 + i * CBSTEP) * 32 < H) {  // wave-uniform: columns < H take their values from the gathered neighbour features
#pragma unroll
                for (int r = 0; r < 16; ++r) vdst[r >> 1][r & 1] = *reinterpret_cast<const float*>(fgb + off[r] + rel);
            }
        };
        gather(0, gq[0], v[0]);
#pragma unroll
        for (int i = 0; i < NCB; ++i) {
            const int cb = cb0 + i * CBSTEP;
            if (i + 1 < NCB) gather(i + 1, gq[(i + 1) & 1], v[(i + 1) & 1]);
            if (i == 0) gstage(2, t0 + t_step);
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
            const float4* wq = reinterpret_cast<const float4*>(wb) + (size_t)cb * NQ * 64 + lane;
            const float* xr = TX + c32 * PITCH + 4 * hl;
#pragma unroll 8
            for (int q = 0; q < NQ; ++q) {
                const float4 ax = *reinterpret_cast<const float4*>(xr + 8 * q);
                const float4 bw = wq[(size_t)q * 64];
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ax.x, bw.x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ax.y, bw.y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ax.z, bw.z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ax.w, bw.w, acc, 0, 0, 0);
            }
            f32x2 (&vv)[8] = v[i & 1];
            const f32x2 (&gs)[8] = gq[i & 1];
#include "att32_tile_pool.h"
        }
        phase_sync();  // the tile and the neighbour rows are overwritten by the next tile
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------
void pack_p32(const float* W, int cin, int cout, float* out)
{
    const int nq = cin / 8, cbs = cout / 32;
    for (int cb = 0; cb < cbs; ++cb)
        for (int q = 0; q < nq; ++q)
            for (int l = 0; l < 64; ++l)
                for (int t = 0; t < 4; ++t)
                    out[((((size_t)cb * nq + q) * 64) + l) * 4 + t] = W[(size_t)(8 * q + 4 * (l >> 5) + t) * cout + 32 * cb + (l & 31)];
}

void pack_p32_locse(const float* W1, int cout, float* out)
{
    const int cbs = cout / 32;
    for (int cb = 0; cb < cbs; ++cb)
        for (int s = 0; s < 5; ++s)
            for (int l = 0; l < 64; ++l) out[((size_t)cb * 5 + s) * 64 + l] = W1[(size_t)(2 * s + (l >> 5)) * cout + 32 * cb + (l & 31)];
}

template <int D, int STAGE, int KN>
static int launch_att32(ps_context* c, const Att32Args& a)
{
    constexpr int H = D / 2, PITCH = H + 4, TILE = 32 * PITCH;
    if constexpr (D <= 128) {
        // d = 128: 52 KB of weights + twelve 8.8 KB tiles = 158 KB: one workgroup of twelve waves per CU (three per SIMD);
        // d = 64: 14 KB + eight 4.7 KB tiles: two workgroups of eight waves per CU (register-limited)
        constexpr int WAVES = D == 128 ? 12 : 8;
        constexpr int PER_CU = D == 128 ? 1 : 2;
        constexpr size_t smem = sizeof(float) * ((size_t)(H / 32) * 5 * 64 + (STAGE == 2 ? H * H : 0) + H * D + 2 * H + (size_t)WAVES * (32 + TILE));
        static_assert(smem <= 160 * 1024, "att32: weights + tiles exceed the LDS");
        auto kern = att32_kernel<D, STAGE, KN, WAVES, false>;
        PS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
        const int tiles = ceil_div(a.n_total, 32 / KN);
        const int blocks = (std::min(ceil_div(tiles, WAVES), 256 * PER_CU) + 7) & ~7;  // persistent: the weights are staged once per workgroup
        hipLaunchKernelGGL(kern, dim3(blocks), dim3(WAVES * 64), smem, c->stream, a);
    } else {
        constexpr int WAVES = D >= 512 ? 8 : 4;
        constexpr size_t smem = sizeof(float) * (32 + (size_t)TILE * (STAGE == 2 ? 2 : 1));
        auto kern = att32_kernel<D, STAGE, KN, WAVES, true>;
        if (smem > 48 * 1024) PS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
        const int tiles = ceil_div(a.n_total, 32 / KN);
        const int blocks = (std::min(tiles, 256 * 16) + 7) & ~7;
        hipLaunchKernelGGL(kern, dim3(blocks), dim3(WAVES * 64), smem, c->stream, a);
    }
    PS_HIP(hipGetLastError());
    return PS_OK;
}

template <int STAGE, int KN>
static int dispatch32(ps_context* c, int d, const Att32Args& a)
{
    switch (d) {
        case 64: return launch_att32<64, STAGE, KN>(c, a);
        case 128: return launch_att32<128, STAGE, KN>(c, a);
        case 256: return launch_att32<256, STAGE, KN>(c, a);
        case 512: return launch_att32<512, STAGE, KN>(c, a);
        default: set_error("att_pool32: d_out %d is not a compiled size (64, 128, 256, 512)", d); return PS_EINVAL;
    }
}

bool att_pool32_fits(const AttStage& s)
{
    // 32-bit byte offsets into fg: rows * (h + d) * 4 bytes must stay below 4 GiB
    return s.p32 && s.wbot && s.d >= 64 && (s.k == 16 || s.k == 32) && s.ldf == s.d / 2 + s.d && s.n_total < (1 << 24) &&
           (uint64_t)s.n_total * (uint64_t)(s.d / 2 + s.d) * 4u < (1ull << 32);
}

int att_pool32_stage(ps_context* c, const AttStage& s)
{
    if (s.n_total <= 0) return PS_OK;
    const Att32Args a = att32_args<Att32Args>(s, s.p32->w1, s.p32->w2, s.p32->wb1, s.p32->wb2);
    return att32_stage_k(s, [&](auto stage, auto k) { return dispatch32<stage(), k()>(c, s.d, a); });
}

}  // namespace ps
