// att32_tile.h -- the one tile frame of the three d >= 64 forward attention kernels: att32_kernel (attpool32.hip, fp32 MFMA) and
// att32b_kernel / att32s_kernel (attpool32b.hip, split-bf16 MFMA).  A tile = 32 rows = the K neighbours of PPT = 32 / K points.  The
// frame owns what the three share; the operand path (staging, MFMA loops, barriers, where the geometry pieces are issued) is theirs:
//
//   att32_tile_walk.h  the XCD walk of the tiles and the three-piece prefetch of the next tile's geometry (gstage)
//   att32_tile_row.h   this lane's row of the tile at the top of the tile loop: point, neighbour, enc10
//   att32_tile_pool.h  a 32-column score block -> softmax over the K rows of a point, weighted sum, store to agg
//   below              LocSE operand of the split form, neighbour-row offsets, bias seed and LDS store of a transposed block (macros),
//                      and on the host the argument struct, its fill and the (stage, K) fan-out
//
// The three att32_tile_*.h are text that the kernels include at the place of use, not __forceinline__ function templates: as a function
// the pooling block moved the scalar register count of the K = 16 att32b kernels (42 -> 44), the vector register count of att32s at
// d = 512 (244 -> 254) and put two of those kernels into scratch; included, every kernel compiles to the code it had with the text
// written out (gemm32_frame.h has the same experience).  The small blocks below, each tried alone as a function and as a lambda, changed
// the register allocation of every att32_kernel likewise; as macros they do not.
#pragma once

#include <type_traits>

#include "attpool.h"
#include "mfma_tile.h"
#include "wave_ops.h"

namespace ps {

// W: the element type of the form's weight images (float: pack_p32 / pack_p32_locse, uint4: pack_b3 / pack_b3_locse)
template <class W>
struct Att32ArgsT {
    const float* xyz;
    const int32_t* idx;
    const int32_t* order;
    const float* fg;
    const W* w1; const float* b1;  // LocSE mlp1
    const W* w2; const float* b2;  // LFA mlp2: image of [H, H] (stage 2)
    const W* wb;                   // Wfc[H:, :] (times log2 e): image of [H, D]
    float* agg;
    int n_total, n_cloud;
};

// The four below are macros for the reason given above: text, with `hl` of the kernel in scope.  Even the order of their address sums and
// the local col0 are load-bearing for "the same code as before": leave them.
// enc10 = [dis, rx, ry, rz, cx, cy, cz, nx | ny, nz] (att32_tile_row.h) as the one K = 16 chunk of the split form, float[8] for b3_split8:
// the lower lane half holds K values 0..7, the upper 8..15 (10.. are zero)
#define ATT32_LOCSE_K16(enc)                                                                                             \
    {hl ? enc[8] : enc[0], hl ? enc[9] : enc[1], hl ? 0.f : enc[2], hl ? 0.f : enc[3],                                   \
     hl ? 0.f : enc[4],    hl ? 0.f : enc[5],    hl ? 0.f : enc[6], hl ? 0.f : enc[7]}
// Accumulator register r of a score tile (C[row][channel]) is row (r & 3) + 8 * (r >> 2) + 4 * hl.  off[r] = byte offset of (that row's
// neighbour in NB, byte column col0) in fg; the column blocks that follow are compile-time byte offsets of the loads (instruction
// immediates): no address arithmetic per gather.  Rows < 2^24 and 32-bit byte offsets: att_pool32_fits.
#define ATT32_ROW_OFFSETS(off, NB, LDF, col0_expr)                                                                       \
    {                                                                                                                    \
        const unsigned col0 = col0_expr;                                                                                 \
        _Pragma("unroll") for (int g4 = 0; g4 < 4; ++g4) {                                                               \
            const int4 nb4 = *reinterpret_cast<const int4*>((NB) + 8 * g4 + 4 * hl);                                     \
            off[4 * g4] = __umul24(nb4.x, (LDF) * 4u) + col0; off[4 * g4 + 1] = __umul24(nb4.y, (LDF) * 4u) + col0;      \
            off[4 * g4 + 2] = __umul24(nb4.z, (LDF) * 4u) + col0; off[4 * g4 + 3] = __umul24(nb4.w, (LDF) * 4u) + col0;  \
        }                                                                                                                \
    }
// Register r of a transposed block (C[channel][row]) = channel 32 cb + 8 (r >> 2) + 4 hl + (r & 3) of the lane's row: four consecutive
// registers are four consecutive channels.  Seed of the accumulator of block cb = the bias (16-byte reads) ...
#define ATT32_BIAS_SEED(acc, b, cb)                                                                                      \
    _Pragma("unroll") for (int g4 = 0; g4 < 4; ++g4) {                                                                   \
        const float4 bb = *reinterpret_cast<const float4*>((b) + (cb) * 32 + g4 * 8 + hl * 4);                           \
        acc[4 * g4] = bb.x; acc[4 * g4 + 1] = bb.y; acc[4 * g4 + 2] = bb.z; acc[4 * g4 + 3] = bb.w;                      \
    }
// ... and its way into the lane's row of an LDS tile (16-byte writes; act: leaky02, or empty for values as they are)
#define ATT32_STORE_BLOCK(row, cb, act, f)                                                                               \
    _Pragma("unroll") for (int g4 = 0; g4 < 4; ++g4) {                                                                   \
        float4 o;                                                                                                        \
        o.x = act(f[4 * g4]); o.y = act(f[4 * g4 + 1]); o.z = act(f[4 * g4 + 2]); o.w = act(f[4 * g4 + 3]);              \
        *reinterpret_cast<float4*>((row) + (cb) * 32 + g4 * 8 + hl * 4) = o;                                             \
    }

// ---- host side -----------------------------------------------------------------------------------------------------------------
// w1 .. wb2: the form's four images of the level (Att32Weights)
template <class Args>
inline Args att32_args(const AttStage& s, const float* w1, const float* w2, const float* wb1, const float* wb2)
{
    using wptr = decltype(Args::w1);
    Args a;
    a.xyz = s.xyz; a.idx = s.idx; a.order = s.order; a.fg = s.fg;
    a.w1 = reinterpret_cast<wptr>(w1); a.b1 = s.lfa1->bias;
    a.w2 = s.lfa2 ? reinterpret_cast<wptr>(w2) : nullptr; a.b2 = s.lfa2 ? s.lfa2->bias : nullptr;
    a.wb = reinterpret_cast<wptr>(s.lfa2 ? wb2 : wb1);
    a.agg = s.agg;
    a.n_total = (int)s.n_total; a.n_cloud = (int)s.n_cloud;
    return a;
}

// launch(stage, k) with the level's stage (2 with LFA mlp2, else 1) and K as std::integral_constant: the four compiled combinations
template <class F>
inline int att32_stage_k(const AttStage& s, F&& launch)
{
    const std::integral_constant<int, 1> s1; const std::integral_constant<int, 2> s2;
    const std::integral_constant<int, 16> k16; const std::integral_constant<int, 32> k32;
    const int stage = s.lfa2 ? 2 : 1;
    if (s.k == 16) return stage == 1 ? launch(s1, k16) : launch(s2, k16);
    return stage == 1 ? launch(s1, k32) : launch(s2, k32);
}

}  // namespace ps
