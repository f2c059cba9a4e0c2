// attpool32b.hip -- attpool32.hip's computation with every matrix product on v_mfma_f32_32x32x16_bf16 over EXACT three-way
// bfloat16 splits of the fp32 operands ("bf16x3").
//
//   x = x1 + x2 + x3,  x1 = x with the low 16 bits cleared, x2 = (x - x1) with the low 16 bits cleared, x3 = x - x1 - x2:
//   each piece has 8 significant bits, the subtractions are exact, and 8 + 8 + 8 = the 24 bits of an fp32 significand -- the
//   three bfloat16 values add up to x exactly.  A product of two pieces is exact in fp32, the MFMA accumulates in fp32, and of the
//   nine piece products the six of relative size >= 2^-16 are kept:  x.w ~ x1w1 + x1w2 + x2w1 + x1w3 + x3w1 + x2w2 (dropped:
//   x2w3 + x3w2 + x3w3 <= 2^-23 |x||w|, the size of ONE fp32 rounding of the product).  The result carries fp32-level error --
//   the logits parity against the float64 oracle is unchanged (tests/test_gpu_network.py) -- while six 32-cycle bf16 MFMAs cover
//   K = 16 where the fp32 MFMA needs eight 64-cycle ones: 2.7 x less matrix-pipe time.  (The fp32 MFMA is 1/16 of the bf16 rate
//   on gfx950, MI355X_MICROARCH.md.)
//
// What changes against attpool32.hip besides the instruction:
//   * activations never go through LDS as operands: the accumulator registers of a transposed product (C[channel][row]) ARE the
//     next product's operand registers of the same lane (tile row = lane & 31, eight K values per lane half) -- LeakyReLU, split,
//     done; the K axis of every product is simply taken in accumulator order (host images packed to match, pack_b3).  The fp32
//     tile in LDS only serves the value reads of the weighted sum.
//   * weights are stored as three planes of eight bfloat16 per lane (16-byte reads, [block][chunk][plane][lane]).
// d = 64 and 128 (levels 1-2): weights resident in LDS, a wave per tile of two points (att32b_kernel);
// d = 256 and 512 (levels 3-4): a workgroup per tile, weight planes streamed from L2 (att32s_kernel).
// What does not change is att32_tile.h's, one text for the three kernels: the tile walk and the geometry prefetch, the neighbour-row
// offsets, bias seed and tile store of a transposed block, and the pooling of a score block.
// The split, the planes and the six-product MFMA are b3_ops.h's (one definition for all bf16x3 kernels); swap32_* are wave_ops.h's.
#include "att32_tile.h"
#include "b3_ops.h"

namespace ps {

struct Att32bArgs : Att32ArgsT<uint4> {};  // w1: pack_b3_locse image; w2, wb: pack_b3 images

// fg as a raw buffer of `bytes` bytes (descriptor from kernel arguments only: wave-uniform, four scalar registers) and one float of it at
// a 32-bit byte offset: buffer_load_dword with the offset register as it is, a constant part of `off` in the instruction's immediate
__device__ __forceinline__ __amdgpu_buffer_rsrc_t fg_rsrc(const float* fg, unsigned bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(fg), 0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ float fg_load(__amdgpu_buffer_rsrc_t r, unsigned off)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, (int)off, 0, 0));
}

// (P = 3 written out as it always was: as a loop over the planes the split kernels of d >= 256 compiled to other code, with more registers)
template <int P>
__device__ __forceinline__ BPlanes<P> load_planes(const uint4* img, int slot, int lane);
template <>
__device__ __forceinline__ B3Planes load_planes<3>(const uint4* img, int slot, int lane)
{
    B3Planes r;
    r.p[0] = img[(slot * 3 + 0) * 64 + lane];
    r.p[1] = img[(slot * 3 + 1) * 64 + lane];
    r.p[2] = img[(slot * 3 + 2) * 64 + lane];
    return r;
}
template <>
__device__ __forceinline__ BPlanes<1> load_planes<1>(const uint4* img, int slot, int lane)
{
    BPlanes<1> r;
    r.p[0] = img[slot * 64 + lane];
    return r;
}

// Staging of an image of N uint4 by NT threads through registers: trip j is element tid + j NT.  A trip that only some threads take
// (the last, when NT does not divide N) loads a clamped index -- an unconditional load stays a register -- and guards its write.
template <int N, int NT, int R>
__device__ __forceinline__ void stage_load(uint4 (&r)[R], const uint4* __restrict__ src, int tid)
{
#pragma unroll
    for (int j = 0; j * NT < N; ++j) r[j] = src[(j + 1) * NT <= N ? tid + j * NT : min(tid + j * NT, N - 1)];
}
template <int N, int NT, bool WHOLE, int R>  // WHOLE: the trips every thread takes; else the partial one
__device__ __forceinline__ void stage_write(uint4* dst, const uint4 (&r)[R], int tid)
{
#pragma unroll
    for (int j = 0; j * NT < N; ++j) {
        if ((j + 1) * NT <= N) {
            if (WHOLE) dst[tid + j * NT] = r[j];
        } else if (!WHOLE && tid + j * NT < N) dst[tid + j * NT] = r[j];
    }
}

// P = 3: the exact split.  P = 1 (PS_PREC_BF16): LFA mlp2 and the score product f_xyz . Wfc[H:, :] take both operands rounded once to bfloat16 --
// one plane per operand, one MFMA per chunk, w2 / wb as one-plane images; the LocSE product keeps the exact split of both operands (w1 stays the
// three-plane pack_b3_locse image): positions at 8 bits would quantise the volume.
template <int D, int STAGE, int KN, int WAVES, int P>
__global__ __launch_bounds__(WAVES * 64) void att32b_kernel(Att32bArgs a)
{
    constexpr int H = D / 2, LDF = H + D, PITCH = H + 4, PPT = 32 / KN;
    constexpr int CBH = H / 32, CBD = D / 32, NQ = H / 16;
    constexpr int W1Q = CBH * 3 * 64, W2Q = STAGE == 2 ? CBH * NQ * P * 64 : 0, WBQ = CBD * NQ * P * 64;  // uint4 counts
    constexpr int TILE = 32 * PITCH;
    static_assert(H % 32 == 0 && (KN == 16 || KN == 32), "att32b: d_out >= 64, K in {16, 32}");

    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int hl = lane >> 5, c32 = lane & 31;
    // LDS: [weight planes | biases] [per wave: 32 neighbour rows | fp32 tile]
    uint4* Wq = reinterpret_cast<uint4*>(smem);
    constexpr int WTOT = (W1Q + W2Q + WBQ) * 4 + 2 * H;  // floats
    float* own = smem + WTOT + wave * (32 + TILE);
    int* NB = reinterpret_cast<int*>(own);
    float* T1 = own + 32;
    // Staging: a thread's 16-byte loads of the three images are requested before the first LDS write (d = 128, stage 2: 1 + 3 + 6 of
    // 512 threads; d = 64: one each) -- written as `Wq[i] = a.w1[i]` loops they were one load, one wait and one write per trip, ten
    // dependent L2 round trips in front of the first tile.  The writes of the trips that every thread takes are one basic block with
    // their loads (nine in flight at d = 128, stage 2); the compiler moves the load of a partial trip (d = 128: 384 uint4 of w1 over
    // 512 threads) into the guarded block of its write, a round trip of its own: two in all.
    {
        constexpr int NT = WAVES * 64;
        constexpr int N1 = (W1Q + NT - 1) / NT, N2 = (W2Q + NT - 1) / NT, NB3 = (WBQ + NT - 1) / NT;
        static_assert(N1 + N2 + NB3 <= 12, "att32b: the staging loads of a thread are held in registers");
        const int tid = threadIdx.x;
        uint4 r1[N1], r2[N2 ? N2 : 1], rb[NB3];
        stage_load<W1Q, NT>(r1, a.w1, tid);
        stage_load<W2Q, NT>(r2, a.w2, tid);
        stage_load<WBQ, NT>(rb, a.wb, tid);
        stage_write<W1Q, NT, true>(Wq, r1, tid);
        stage_write<W2Q, NT, true>(Wq + W1Q, r2, tid);
        stage_write<WBQ, NT, true>(Wq + W1Q + W2Q, rb, tid);
        stage_write<W1Q, NT, false>(Wq, r1, tid);
        stage_write<W2Q, NT, false>(Wq + W1Q, r2, tid);
        stage_write<WBQ, NT, false>(Wq + W1Q + W2Q, rb, tid);
    }
    float* bias = smem + (W1Q + W2Q + WBQ) * 4;
    for (int i = threadIdx.x; i < H; i += WAVES * 64) {
        bias[i] = a.b1[i];
        bias[H + i] = STAGE == 2 ? a.b2[i] : 0.f;
    }
    __syncthreads();
    const uint4 *w1 = Wq, *w2 = Wq + W1Q, *wb = Wq + W1Q + W2Q;
    const float *b1 = bias, *b2 = bias + H;

    constexpr int TPW = WAVES;
    const int tiw = wave;
    const __amdgpu_buffer_rsrc_t fgr = fg_rsrc(a.fg, (unsigned)a.n_total * (unsigned)(LDF * 4));
#include "att32_tile_walk.h"
    for (int t0 = t_first; t0 < t_end; t0 += t_step) {
#include "att32_tile_row.h"
        const float ev[8] = ATT32_LOCSE_K16(enc);
        const B3Planes E = b3_split8<3>(ev);
        if (hl == 0) NB[c32] = nbr;
        gstage(0, t0 + t_step);
        wave_lds_sync();
        unsigned off[16];  // of this lane's column of the first column block
        ATT32_ROW_OFFSETS(off, NB, LDF, (unsigned)c32 * 4u);
        // The gathers of the later blocks are issued in other basic blocks than the one that computes off[] (gstage and the guarded stores
        // of the pooling split the tile), and as `fgb + off[r] + rel` only the FIRST block's loads were selected in the scalar-base +
        // 32-bit-offset form: the sum base + zext(off[r]) is hoisted as ONE 64-bit value, and a later block sees a 64-bit pointer, not
        // the zero-extension (d = 64: 16 of 48 gathers with a v_lshl_add_u64 and a zero high half each; d = 128: 64 of 96).  A raw buffer
        // load takes the 32-bit offset as such wherever it is issued; the range of the descriptor is fg's n_total rows of LDF floats
        // (32-bit byte offsets: att_pool32_fits).
        f32x2 gq[2][8], v[2][8];
        auto gather = [&](int i, f32x2 (&gdst)[8], f32x2 (&vdst)[8]) {
            const int rel = i * 32 * 4;  // compile-time (the loop below is fully unrolled): the instruction's immediate
#pragma unroll
            for (int r = 0; r < 16; ++r) gdst[r >> 1][r & 1] = fg_load(fgr, off[r] + (rel + H * 4));
            if (i * 32 < H) {
#pragma unroll
                for (int r = 0; r < 16; ++r) vdst[r >> 1][r & 1] = fg_load(fgr, off[r] + rel);
            }
        };
        gather(0, gq[0], v[0]);  // the first block's G and value rows travel under the two small products

        // ---- LFA mlp1 (transposed: C[channel][row]): f_xyz1 = lrelu(enc10 . W1 + b1) ----
        // register r of this lane = channel 32 cb + 8 (r >> 2) + 4 hl + (r & 3) of row c32
        f32x16 f1[CBH];
#pragma unroll
        for (int cb = 0; cb < CBH; ++cb) {
            f32x16 acc;
            ATT32_BIAS_SEED(acc, b1, cb);
            acc = b3_mfma6<3>(load_planes<3>(w1, cb, lane), E, acc);
#pragma unroll
            for (int r = 0; r < 16; ++r) f1[cb][r] = leaky02(acc[r]);
        }
        gstage(1, t0 + t_step);
        BPlanes<P> PL[NQ];  // the operand planes of the tile that feeds the scores (chunk q = accumulator registers 8 (q & 1) .. of block q >> 1)
        auto split_block = [&](const f32x16& f, BPlanes<P>& lo, BPlanes<P>& hi) {
            const float x0[8] = {f[0], f[1], f[2], f[3], f[4], f[5], f[6], f[7]};
            const float x1[8] = {f[8], f[9], f[10], f[11], f[12], f[13], f[14], f[15]};
            lo = b3_split8<P>(x0);
            hi = b3_split8<P>(x1);
        };
        auto store_block = [&](const f32x16& f, int cb) {  // -> fp32 tile (value reads of the weighted sum)
            ATT32_STORE_BLOCK(T1 + c32 * PITCH, cb, , f);
        };
#pragma unroll
        for (int cb = 0; cb < CBH; ++cb) split_block(f1[cb], PL[2 * cb], PL[2 * cb + 1]);
        if constexpr (STAGE == 1) {
#pragma unroll
            for (int cb = 0; cb < CBH; ++cb) store_block(f1[cb], cb);
        } else {
            // ---- LFA mlp2 (transposed): f_xyz2 = lrelu(f_xyz1 . W2 + b2); the planes of f_xyz1 are the B operands ----
            f32x16 f2[CBH];
#pragma unroll
            for (int cb = 0; cb < CBH; ++cb) {
                f32x16 acc;
                ATT32_BIAS_SEED(acc, b2, cb);
#pragma unroll
                for (int q = 0; q < NQ; ++q) acc = b3_mfma6<P>(load_planes<P>(w2, cb * NQ + q, lane), PL[q], acc);
#pragma unroll
                for (int r = 0; r < 16; ++r) f2[cb][r] = leaky02(acc[r]);
            }
#pragma unroll
            for (int cb = 0; cb < CBH; ++cb) {
                split_block(f2[cb], PL[2 * cb], PL[2 * cb + 1]);
                store_block(f2[cb], cb);
            }
        }
        wave_lds_sync();
        const float* TX = T1;

        // ---- scores (C[row][channel]) = G[nbr] + f_xyz . Wfc[H:, :], softmax over the K rows of a point, weighted sum ----
#pragma unroll
        for (int cb = 0; cb < CBD; ++cb) {
            if (cb + 1 < CBD) gather(cb + 1, gq[(cb + 1) & 1], v[(cb + 1) & 1]);
            if (cb == 0) gstage(2, t0 + t_step);
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
            for (int q = 0; q < NQ; ++q) acc = b3_mfma6<P>(PL[q], load_planes<P>(wb, cb * NQ + q, lane), acc);
            f32x2 (&vv)[8] = v[cb & 1];
            const f32x2 (&gs)[8] = gq[cb & 1];
#include "att32_tile_pool.h"
        }
        wave_lds_sync();  // the tile and the neighbour rows are overwritten by the next tile
    }
}


// ---- d >= 256 (levels 3-4: few points): the waves of a workgroup share one tile and split its column blocks; the weight planes
// stream from L2 (16-byte loads, one stage ahead), the tile's operand planes go through LDS ([chunk][plane][lane], 16 bytes per lane:
// every wave needs all chunks but produces only its own blocks).  Each wave runs its two score blocks together, so an operand
// plane read from LDS feeds both.
// (P as in att32b_kernel: one plane for LFA mlp2 and the score product, the LocSE product on the exact split)
template <int D, int STAGE, int KN, int WAVES, int P>
__global__ __launch_bounds__(WAVES * 64) void att32s_kernel(Att32bArgs a)
{
    constexpr int H = D / 2, LDF = H + D, PITCH = H + 4, PPT = 32 / KN;
    constexpr int CBH = H / 32, CBD = D / 32, NQ = H / 16;
    constexpr int PLQ = NQ * P * 64;  // uint4s of one set of operand planes
    constexpr int NB_H = CBH / WAVES, NB_D = CBD / WAVES;  // blocks per wave
    static_assert(CBH % WAVES == 0 && NB_D == 2 && (KN == 16 || KN == 32), "att32s: two score blocks per wave");

    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;  // (kept in a VGPR here: as an SGPR this kernel measured 8-22 % slower)
    const int hl = lane >> 5, c32 = lane & 31;
    // LDS: [32 neighbour rows] [operand planes A] [operand planes B (stage 2)] [fp32 value tile]
    int* NB = reinterpret_cast<int*>(smem);
    uint4* PA = reinterpret_cast<uint4*>(smem + 32);
    uint4* PB = STAGE == 2 ? PA + PLQ : PA;
    float* TX = reinterpret_cast<float*>(PB + PLQ);

    constexpr int TPW = 1;  // the waves of a workgroup share one tile
    const int tiw = 0;
#include "att32_tile_walk.h"
    auto seed = [&](const float* b, int cb) {  // (as a lambda: written out in place this kernel compiles to other code)
        f32x16 acc;
        ATT32_BIAS_SEED(acc, b, cb);
        return acc;
    };
    // LeakyReLU of a transposed block -> its two chunks of operand planes (LDS) and, when asked, the fp32 value tile
    auto emit_block = [&](const f32x16& acc, int cb, uint4* planes, bool values) {
        float x0[8], x1[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) { x0[r] = leaky02(acc[r]); x1[r] = leaky02(acc[8 + r]); }
        const BPlanes<P> lo = b3_split8<P>(x0), hi = b3_split8<P>(x1);
#pragma unroll
        for (int pl = 0; pl < P; ++pl) {
            planes[((2 * cb) * P + pl) * 64 + lane] = lo.p[pl];
            planes[((2 * cb + 1) * P + pl) * 64 + lane] = hi.p[pl];
        }
        if (values) {  // (ATT32_STORE_BLOCK from x0 | x1)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const float* x = g4 < 2 ? x0 + 4 * g4 : x1 + 4 * (g4 - 2);
                *reinterpret_cast<float4*>(TX + c32 * PITCH + cb * 32 + g4 * 8 + hl * 4) = make_float4(x[0], x[1], x[2], x[3]);
            }
        }
    };
    static_assert(NB_H == 1, "att32s: one transposed block per wave");
    const B3Planes W1 = load_planes<3>(a.w1, wave, lane);  // this wave's LocSE block: resident for the whole kernel
    const f32x16 seed1 = seed(a.b1, wave);
    // P = 3: score-weight chunks in flight per block (measured: 2 at d = 256, 4 at d = 512) and mlp2-weight chunks in flight (measured: all 8
    // at d = 256, 4 at d = 512).  P = 1: a chunk is 1 KB per wave instead of 3 and its product one MFMA instead of six, so the same bytes in
    // flight against the same L2 latency are three times the chunks.  d = 256: all eight chunks of a block in both rings (16 + 8 uint4 per lane,
    // 202-220 registers).  d = 512: eight spilled (76-236 bytes of scratch per lane next to the 32 accumulators of two score blocks and the 32
    // gathered values); six does not divide the sixteen chunks of a block, so four, the split form's depth at a third of its registers.
    // Reasoned from the sizes and the compiler's resource summary, not measured.
    constexpr int PD = P == 1 ? (D >= 512 ? 4 : 8) : (D >= 512 ? 4 : 2);
    constexpr int PD2 = STAGE == 2 ? (D >= 512 ? 4 : 8) : 1;  // (the same depths at P = 1, for the reasons above)
    static_assert(NQ % PD == 0 && (STAGE == 1 || NQ % PD2 == 0), "att32s: the rings walk the K axis in whole passes");
    const int cbA = wave, cbB = wave + WAVES;
    for (int t0 = t_first; t0 < t_end; t0 += t_step) {
#include "att32_tile_row.h"
        const float ev[8] = ATT32_LOCSE_K16(enc);
        const B3Planes E = b3_split8<3>(ev);
        if (hl == 0 && wave == 0) NB[c32] = nbr;
        gstage(0, t0 + t_step);
        // the first weight chunks of the next product do not depend on anything: they travel under LocSE and its barrier
        BPlanes<P> ring[PD2], rA[PD], rB[PD];
        if constexpr (STAGE == 2) {
#pragma unroll
            for (int q = 0; q < PD2; ++q) ring[q] = load_planes<P>(a.w2, wave * NQ + q, lane);
        } else {
#pragma unroll
            for (int q = 0; q < PD; ++q) {
                rA[q] = load_planes<P>(a.wb, cbA * NQ + q, lane);
                rB[q] = load_planes<P>(a.wb, cbB * NQ + q, lane);
            }
        }

        // ---- LFA mlp1 (transposed), this wave's block ----
        emit_block(b3_mfma6<3>(W1, E, seed1), wave, PA, STAGE == 1);
        __syncthreads();
        gstage(1, t0 + t_step);
        // neighbour-row offsets and the gathers of this wave's two score blocks (they travel under the products below)
        unsigned off[16];
        ATT32_ROW_OFFSETS(off, NB, LDF, (unsigned)(wave * 32 + c32) * 4u);
        const char* fgb = reinterpret_cast<const char*>(a.fg);
        if constexpr (STAGE == 2) {
            // ---- LFA mlp2 (transposed): weights (A) stream from L2 PD2 chunks ahead, f_xyz1's planes (B) come from LDS ----
            const int cb = wave;
            f32x16 acc = seed(a.b2, cb);
#pragma unroll 1
            for (int q0 = 0; q0 + PD2 < NQ; q0 += PD2) {
#pragma unroll
                for (int j = 0; j < PD2; ++j) {
                    acc = b3_mfma6<P>(ring[j], load_planes<P>(PA, q0 + j, lane), acc);
                    ring[j] = load_planes<P>(a.w2, cb * NQ + q0 + j + PD2, lane);  // refilled in place, behind its last reader
                }
            }
#pragma unroll
            for (int j = 0; j < PD2; ++j) acc = b3_mfma6<P>(ring[j], load_planes<P>(PA, NQ - PD2 + j, lane), acc);
#pragma unroll
            for (int q = 0; q < PD; ++q) {  // the score product's first chunks, under the split + barrier
                rA[q] = load_planes<P>(a.wb, cbA * NQ + q, lane);
                rB[q] = load_planes<P>(a.wb, cbB * NQ + q, lane);
            }
            emit_block(acc, cb, PB, true);
            __syncthreads();
        }
        gstage(2, t0 + t_step);

        // ---- scores of this wave's two column blocks, softmax over the K rows of a point, weighted sum ----
        f32x16 accA, accB;
#pragma unroll
        for (int r = 0; r < 16; ++r) { accA[r] = 0.f; accB[r] = 0.f; }
        f32x2 gq[2][8], v[2][8];
        {
#pragma unroll 1
            for (int q0 = 0; q0 + PD < NQ; q0 += PD) {
#pragma unroll
                for (int j = 0; j < PD; ++j) {
                    const BPlanes<P> x = load_planes<P>(PB, q0 + j, lane);
                    accA = b3_mfma6<P>(x, rA[j], accA);
                    accB = b3_mfma6<P>(x, rB[j], accB);
                    rA[j] = load_planes<P>(a.wb, cbA * NQ + q0 + j + PD, lane);  // refilled in place, behind its last reader
                    rB[j] = load_planes<P>(a.wb, cbB * NQ + q0 + j + PD, lane);
                }
            }
            // last pass: nothing is refilled any more; the G rows of both blocks travel under its products
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) gq[i][r >> 1][r & 1] = *reinterpret_cast<const float*>(fgb + off[r] + (i * WAVES * 32 * 4 + H * 4));
#pragma unroll
            for (int j = 0; j < PD; ++j) {
                const BPlanes<P> x = load_planes<P>(PB, NQ - PD + j, lane);
                accA = b3_mfma6<P>(x, rA[j], accA);
                accB = b3_mfma6<P>(x, rB[j], accB);
            }
        }
        // value rows of the first block (columns < H: gathered neighbour features); the second block (f_xyz columns, LDS) goes first
#pragma unroll
        for (int r = 0; r < 16; ++r) v[0][r >> 1][r & 1] = *reinterpret_cast<const float*>(fgb + off[r]);
#pragma unroll
        for (int ii = 0; ii < 2; ++ii) {
            const int i = 1 - ii;
            const int cb = wave + i * WAVES;
            const f32x16& acc = i == 0 ? accA : accB;
            f32x2 (&vv)[8] = v[i];
            const f32x2 (&gs)[8] = gq[i];
#include "att32_tile_pool.h"
        }
        __syncthreads();  // planes, value tile and neighbour rows are overwritten by the next tile
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------
// K order of an operand that comes out of a transposed product's accumulators: chunk q, lane half g, element j
static inline int kmap(int q, int g, int j)
{
    const int r = 8 * (q & 1) + j;
    return 32 * (q >> 1) + (r & 3) + 8 * (r >> 2) + 4 * g;
}

void pack_b3(const float* W, int cin, int cout, uint16_t* out, int planes)  // planes = 1: the weights rounded to nearest even, 2 bytes each
{
    const int nq = cin / 16, cbs = cout / 32;
    for (int cb = 0; cb < cbs; ++cb)
        for (int q = 0; q < nq; ++q)
            for (int pl = 0; pl < planes; ++pl)
                for (int l = 0; l < 64; ++l)
                    for (int j = 0; j < 8; ++j)
                        out[(((((size_t)cb * nq + q) * planes + pl) * 64 + l) * 8) + j] =
                            b3_plane_of(W[(size_t)kmap(q, l >> 5, j) * cout + 32 * cb + (l & 31)], pl, planes);
}

void pack_b3_locse(const float* W1, int cout, uint16_t* out)
{
    const int cbs = cout / 32;
    for (int cb = 0; cb < cbs; ++cb)
        for (int pl = 0; pl < 3; ++pl)
            for (int l = 0; l < 64; ++l)
                for (int j = 0; j < 8; ++j) {
                    const int k = 8 * (l >> 5) + j;
                    out[((((size_t)cb * 3 + pl) * 64 + l) * 8) + j] = k < 10 ? b3_piece_of(W1[(size_t)k * cout + 32 * cb + (l & 31)], pl) : (uint16_t)0;
                }
}

template <int D, int STAGE, int KN, int P>
static int launch_att32b(ps_context* c, const Att32bArgs& a)
{
    constexpr int H = D / 2, PITCH = H + 4, TILE = 32 * PITCH;
    constexpr int CBH = H / 32, CBD = D / 32, NQ = H / 16;
    // d = 128: 78 KB of weight planes + eight 8.8 KB tiles = 148 KB: one workgroup of eight waves per CU; d = 64: 21 KB + twelve 4.7 KB
    // tiles, one workgroup of twelve waves (134 registers: three waves per SIMD) in stage 2
    // (d = 64, stage 1: sixteen waves -- 126 registers, four waves per SIMD: 43.5 -> 41.2 us; stage 2 needs 134 and spills at sixteen: 50.0 -> 51.0)
    // (with the gathers as buffer loads the counts are 116 and 124: sixteen waves would fit stage 2 now -- not measured)
    // P = 1, derived from its own sizes: d = 128: 6 KB of LocSE planes + 8 + 16 KB of one-plane images = 30 KB, twelve 8.8 KB tiles = 136 KB (sixteen
    // would be 171 KB); d = 64: 9 KB + sixteen 4.7 KB tiles = 84 KB in both stages.  The operand planes of a tile are a third of the split form's
    // (d = 128: 16 registers for 48), which is what lets stage 2 keep the register budget of twelve (168) and sixteen (128) waves: the compiler's
    // resource summary shows no scratch for any of them
    constexpr int WAVES = P == 1 ? (D == 128 ? 12 : 16) : (D == 128 ? 8 : (STAGE == 1 ? 16 : 12));
    constexpr int PER_CU = 1;
    constexpr size_t planes = (size_t)(CBH * 3 + ((STAGE == 2 ? CBH * NQ : 0) + CBD * NQ) * P) * 64 * 16;
    constexpr size_t smem = planes + sizeof(float) * (2 * H + (size_t)WAVES * (32 + TILE));
    static_assert(smem <= 160 * 1024, "att32b: weights + tiles exceed the LDS");
    auto kern = att32b_kernel<D, STAGE, KN, WAVES, P>;
    PS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    const int tiles = ceil_div(a.n_total, 32 / KN);
    const int blocks = (std::min(ceil_div(tiles, WAVES), 256 * PER_CU) + 7) & ~7;
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(WAVES * 64), smem, c->stream, a);
    PS_HIP(hipGetLastError());
    return PS_OK;
}

template <int D, int STAGE, int KN, int P>
static int launch_att32s(ps_context* c, const Att32bArgs& a)
{
    constexpr int H = D / 2, PITCH = H + 4, NQ = H / 16;
    constexpr int WAVES = D / 64;  // two score blocks per wave: 4 waves at d = 256, 8 at d = 512
    constexpr size_t smem = sizeof(float) * 32 + (size_t)(STAGE == 2 ? 2 : 1) * NQ * P * 64 * 16 + sizeof(float) * 32 * PITCH;
    static_assert(smem <= 160 * 1024, "att32s: planes + value tile exceed the LDS");
    auto kern = att32s_kernel<D, STAGE, KN, WAVES, P>;
    if (smem > 48 * 1024) PS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    const int tiles = ceil_div(a.n_total, 32 / KN);
    const int blocks = (std::min(tiles, 256 * 16) + 7) & ~7;
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(WAVES * 64), smem, c->stream, a);
    PS_HIP(hipGetLastError());
    return PS_OK;
}

bool att_pool32b_fits(const AttStage& s)
{
    return att_pool32_fits(s) && s.p32->w1b && (s.d == 64 || s.d == 128 || s.d == 256 || s.d == 512);
}

template <int P>
static int att32b_stage_p(ps_context* c, const AttStage& s, const Att32bArgs& a)
{
    if (s.d == 64) return att32_stage_k(s, [&](auto stage, auto k) { return launch_att32b<64, stage(), k(), P>(c, a); });
    if (s.d == 128) return att32_stage_k(s, [&](auto stage, auto k) { return launch_att32b<128, stage(), k(), P>(c, a); });
    if (s.d == 256) return att32_stage_k(s, [&](auto stage, auto k) { return launch_att32s<256, stage(), k(), P>(c, a); });
    return att32_stage_k(s, [&](auto stage, auto k) { return launch_att32s<512, stage(), k(), P>(c, a); });
}

int att_pool32b_stage(ps_context* c, const AttStage& s)
{
    if (s.n_total <= 0) return PS_OK;
    if (s.one_plane) {  // PS_PREC_BF16: LFA mlp2 and the score product on one plane of rounded operands; LocSE on its three-plane image
        PS_CHECK(s.p32->wb1b1 && s.p32->wb2b1 && s.p32->w2b1, "att_pool32b: the level has no one-plane images");
        return att32b_stage_p<1>(c, s, att32_args<Att32bArgs>(s, s.p32->w1b, s.p32->w2b1, s.p32->wb1b1, s.p32->wb2b1));
    }
    return att32b_stage_p<3>(c, s, att32_args<Att32bArgs>(s, s.p32->w1b, s.p32->w2b, s.p32->wb1b, s.p32->wb2b));
}

}  // namespace ps
