// attpool_gemm_kit.h -- the steps of the training step's attentive pooling on v_mfma_f32_32x32x16_bf16 (attpool_gemm.hip), each written
// once: the lane's place in a 32x32 accumulator tile, the weight-block stream of a workgroup and its staging registers, the row source
// (materialised, split-source, bfloat16 rows), the score product of a panel, the softmax / weighted sum / dS step of a point's scores,
// the transposing product, and the dF tile stores.  Everything is forced inline and takes its state as parameters or members: the
// kernels keep their own bodies (tile ownership, order of the products, prefetch distance, every sched_barrier).
#pragma once

#include "common.h"
#include <type_traits>
#include "mfma_tile.h"
#include "b3_ops.h"
#include "bf16_io.h"

namespace ps {

struct AttGArgs {
    const float* f; int ld;    // [rows, D] neighbour set, rows = points * 16
    const uint4* w1;           // W planes, natural K order: [D/16][D/32][P][64]
    const uint4* w2;           // W^T planes, accumulator K order (backward)
    const float* dagg;         // [points, D] (backward)
    float* agg;                // [points, D] (forward)
    float* df; int lddf;       // [rows, D] (backward)
    float* ds; int ldds;       // [rows, D] (backward)
    int64_t rows, points;
    int df_accum;              // df += instead of df =
    // split-source form (gather_neighbour + concat folded in, RandLANet.py:326-333): F = [fl[idx] | f] -- `f` / `df` then hold only the
    // right half ([rows, D/2]); the gathered half's gradient leaves as plain rows dfl_rows [rows, D/2] for the gather-reduction
    const float* fl; int ldl;  // [B * n_src, D/2]
    const int32_t* idx;        // [points, 16] cloud-local source rows
    int64_t n_src, n_q;        // rows per cloud of fl / points per cloud
    float* dfl_rows; int ld_rows;
    int f_bf16;                // forward, split form, bf16-MLP mode: the rows of `f` are STORED as bfloat16 (ps_set_train_act_bf16; ld in elements)
};

template <int N, class F>
__device__ __forceinline__ void attg_static_for(F&& f)
{
    if constexpr (N > 0) {
        attg_static_for<N - 1>(f);
        f(std::integral_constant<int, N - 1>{});
    }
}

__device__ __forceinline__ float attg_swap_max(float v)
{
    auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return fmaxf(__uint_as_float(b[0]), __uint_as_float(b[1]));
}
__device__ __forceinline__ float attg_swap_sum(float v)
{
    auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return __uint_as_float(b[0]) + __uint_as_float(b[1]);
}

// ---- a lane in a 32x32 accumulator tile -------------------------------------------------------------------------------------------------
// Register j (0..15) of lane half hl holds row (j & 3) + 8 (j >> 2) + 4 hl of the tile, the lane's c32 is the column: registers 8 pi ..
// 8 pi + 7 of the two lane halves are the 16 rows of point pi.  The same map names the k-slots of an operand taken in accumulator order.
// The lane's part, row0() = 4 hl, is kept apart: an address takes it once (with the column) and steps through the registers by the
// compile-time attg_acc_row(j) -- with both in one expression per register the kernels of d = 64 kept an address register per access.
__device__ __forceinline__ constexpr int attg_acc_row(int j) { return (j & 3) + 8 * (j >> 2); }

struct AttGLane {
    int wave, lane, hl, c32;
    __device__ __forceinline__ AttGLane() : wave(__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)), lane(threadIdx.x & 63), hl(lane >> 5), c32(lane & 31) {}
    __device__ __forceinline__ int row0() const { return 4 * hl; }
    // the row of a 32-row tile this lane holds as the ROW operand of a product (lane = row); `second` = 0: the tile has one point, whose
    // rows are then read twice
    __device__ __forceinline__ int operand_row(int second) const { return c32 < 16 ? c32 : c32 - 16 + second; }
};

// ---- the weight-block stream of a workgroup (d >= 128) ----------------------------------------------------------------------------------
// block = [2 chunks of 16 K][4 column tiles][P planes][64 lanes] uint4 (24 KB at P = 3), cut out of an image [K/16][D/32][P][64] at
// (chunk pair s, tile group g).  Sequence per panel p: the D/32 K-steps of the score product (image w1, group p), then per 32-column tile
// t of the panel and per group ig of four output tiles the blocks of dS . W^T (image w2, chunk pair 4 p + t, group ig).
// HALF (backward of d = 512 only): the launch produces the dF columns [256 HALF, 256 HALF + 256) -- NIG = NPAN / 2 groups of four output
// tiles per (panel, tile) instead of NPAN; -1 = all columns in one launch.
template <int D, int P, bool BWD, int HALF = -1>
struct AttGStream {
    static constexpr int PLANES = P, NCB = D / 32, NPAN = D / 128, STEPS = D / 32;
    static constexpr int NIG = HALF < 0 ? NPAN : NPAN / 2, IG0 = HALF < 0 ? 0 : HALF * NIG;
    static constexpr int PER = BWD ? STEPS + 4 * NIG : STEPS;
    static constexpr int NB = NPAN * PER;
    static constexpr int BLOCK = 2 * 4 * P * 64;  // uint4 per block
    struct Blk {
        const uint4* img;
        int s, g;
    };
    static __device__ __forceinline__ Blk blk(const AttGArgs& a, int n)
    {
        const int p = n / PER, m = n - p * PER;
        if (!BWD || m < STEPS) return Blk{a.w1, m, p};
        const int m2 = m - STEPS, t = m2 / NIG, ig = IG0 + (m2 - t * NIG);
        return Blk{a.w2, 4 * p + t, ig};
    }
    static __device__ __forceinline__ const uint4* src(const Blk& b, int i)  // i in [0, 512 P): (u, rest)
    {
        const int u = i / (256 * P), rest = i - u * (256 * P);
        return b.img + ((size_t)((2 * b.s + u) * NCB + 4 * b.g) * P) * 64 + rest;
    }
};

// a block on its way L2 -> registers -> LDS: 2 P uint4 per thread of the 256
template <class S>
struct AttGStage {
    // (a native vector, not uint4: copies of that struct between address spaces are memcpy calls, behind which an ARRAY stays in scratch)
    using Reg = __attribute__((ext_vector_type(4))) unsigned;
    Reg r[2 * S::PLANES];
    __device__ __forceinline__ void load(const typename S::Blk& b)
    {
#pragma unroll
        for (int i = 0; i < 2 * S::PLANES; ++i) r[i] = *reinterpret_cast<const Reg*>(S::src(b, i * 256 + (int)threadIdx.x));
    }
    __device__ __forceinline__ void store(uint4* bs) const
    {
#pragma unroll
        for (int i = 0; i < 2 * S::PLANES; ++i) *reinterpret_cast<Reg*>(bs + (i * 256 + threadIdx.x)) = r[i];
    }
};

// ---- the rows of a wave -----------------------------------------------------------------------------------------------------------------
// Row addressing: every global access of a wave is (wave-uniform 64-bit base of its 32 rows) + (32-bit lane offset inside them), so no
// 64-bit address arithmetic sits in vector registers.  A wave whose rows end early (the last workgroup) computes on rows that exist --
// a missing second point reads the first one's rows, a wave without rows reads the first 32 -- and stores nothing for them.
struct AttGRows {
    int64_t rbase;   // first row the wave READS
    int nvalid;      // rows of the wave that exist: 0, 16 or 32 (stores)
    int second;      // row offset of the second point's reads: 16, or 0 when only one point is readable
};
__device__ __forceinline__ AttGRows attg_rows(const AttGArgs& a, int wave)
{
    const int64_t row0 = (int64_t)blockIdx.x * 128 + wave * 32;
    AttGRows r;
    const int64_t left = a.rows - row0;
    r.nvalid = left >= 32 ? 32 : (left >= 16 ? 16 : 0);
    r.rbase = r.nvalid > 0 ? row0 : 0;
    r.second = a.rows - r.rbase >= 32 ? 16 : 0;
    return r;
}

// Where a wave's 32 rows come from.  SPLIT: the left half of every row is the gathered source row fl[cloud base + idx[row]], the right half
// the row of `f`.  FRB (split form, one plane): the rows of `f` are bfloat16 -- eight of them ARE a lane's operand fragment (no split, no
// rounding: the sixteen bytes go to the matrix pipe as loaded).
template <int D, bool SPLIT, bool FRB>
struct AttGSource {
    static_assert(!FRB || SPLIT, "bfloat16 rows: split-source form");
    using Row = std::conditional_t<FRB, __bf16, float>;
    const AttGArgs& a;
    const AttGLane& ln;
    const Row* fb;                             // wave-uniform: the wave's first row of `f`
    int second;
    unsigned xoff;                             // the lane's operand row inside them, at its 8-column half of a K chunk
    const float* pL = nullptr;                 // split: the lane's gathered operand row
    const float* flc[2] = {nullptr, nullptr};  // split: the cloud of point pi in fl
    int vidx[2][8] = {};                       // split: the sources of point pi's value rows in accumulator order (two int4, once per kernel)

    __device__ __forceinline__ AttGSource(const AttGArgs& a_, const AttGRows& rw, const AttGLane& ln_)
        : a(a_), ln(ln_), fb(reinterpret_cast<const Row*>(a_.f) + (size_t)rw.rbase * a_.ld), second(rw.second),
          xoff((unsigned)(ln_.operand_row(rw.second) * a_.ld + 8 * ln_.hl))
    {
        if constexpr (SPLIT) {
            const int64_t row = rw.rbase + ln.operand_row(rw.second);
            pL = a.fl + (size_t)(((row >> 4) / a.n_q) * a.n_src + a.idx[row]) * a.ldl + 8 * ln.hl;
#pragma unroll
            for (int pi = 0; pi < 2; ++pi) {
                const int64_t rb = rw.rbase + (pi ? rw.second : 0);
                flc[pi] = a.fl + (size_t)(((rb >> 4) / a.n_q) * a.n_src) * a.ldl;
                const int4 g0 = *reinterpret_cast<const int4*>(a.idx + rb + 4 * ln.hl), g1 = *reinterpret_cast<const int4*>(a.idx + rb + 8 + 4 * ln.hl);
                vidx[pi][0] = g0.x; vidx[pi][1] = g0.y; vidx[pi][2] = g0.z; vidx[pi][3] = g0.w;
                vidx[pi][4] = g1.x; vidx[pi][5] = g1.y; vidx[pi][6] = g1.z; vidx[pi][7] = g1.w;
            }
        }
    }
    // chunk u of K step s (columns 32 s + 16 u ..) of the lane's operand row -> areg
    __device__ __forceinline__ void load_half(int s, int u, float4 (&areg)[4])
    {
        if (SPLIT && 32 * s < D / 2) {  // (a K step lies in one half: D/2 is a multiple of 32)
            areg[2 * u] = *reinterpret_cast<const float4*>(pL + (32 * s + 16 * u));
            areg[2 * u + 1] = *reinterpret_cast<const float4*>(pL + (32 * s + 16 * u + 4));
        } else {
            const Row* p = fb + (xoff + (unsigned)(32 * s - (SPLIT ? D / 2 : 0)));  // (the K step once; the chunk and its halves are constants)
            areg[2 * u] = *reinterpret_cast<const float4*>(p + 16 * u);  // (eight bfloat16 = the fragment itself; kept as loaded)
            if constexpr (!FRB) areg[2 * u + 1] = *reinterpret_cast<const float4*>(p + 16 * u + 4);
        }
    }
    template <int P>
    __device__ __forceinline__ BPlanes<P> planes(int u, int s, const float4 (&areg)[4]) const
    {
        if constexpr (FRB) {
            if (32 * s >= D / 2) {
                BPlanes<P> r;
                r.p[0] = __builtin_bit_cast(uint4, areg[2 * u]);
                return r;
            }
        }
        return b3_split8<P>(areg[2 * u], areg[2 * u + 1]);
    }
    // value rows of (column col, point pi) in accumulator order: fv[j] = row 16 pi + row0() + attg_acc_row(j) of the wave
    __device__ __forceinline__ void values(float (&fv)[8], int col, int pi) const
    {
        if (SPLIT && col < D / 2) {  // gathered half: the rows' sources, column col of each
            const float* vb = flc[pi] + col;
#pragma unroll
            for (int j = 0; j < 8; ++j) fv[j] = vb[(unsigned)vidx[pi][j] * (unsigned)a.ldl];
        } else {  // rows of fp32 or of bfloat16 (the pointer arithmetic in elements)
            const Row* vb = fb + (pi ? second * a.ld : 0) - (SPLIT ? D / 2 : 0);
            const unsigned voff = (unsigned)(ln.row0() * a.ld + col);
#pragma unroll
            for (int j = 0; j < 8; ++j) fv[j] = (float)vb[voff + (unsigned)(attg_acc_row(j) * a.ld)];
        }
    }
};

// ---- the score product of one panel -----------------------------------------------------------------------------------------------------
// acc[t] (t = 0..3) += F[rows of the wave][:] . W[:, 128 p + 32 t ..]; consumes blocks n .. n + STEPS - 1 of the stream (block n is in
// Bs[n & 1] on entry, and block n + STEPS -- if any -- is in Bs[(n + STEPS) & 1] on exit)
template <class S, class Src>
__device__ __forceinline__ void attg_scores(const AttGArgs& a, Src& src, AttGStage<S>& stg, uint4 (&Bs)[2][S::BLOCK], int lane, int& n, f32x16 (&acc)[4])
{
    constexpr int P = S::PLANES;
    float4 areg[4];  // the K step in flight: chunk u = areg[2 u], areg[2 u + 1] (as a member of the source: 130 VGPRs for 128 with bfloat16 rows)
    src.load_half(0, 0, areg);
    src.load_half(0, 1, areg);
#pragma unroll 1
    for (int s = 0; s < S::STEPS; ++s, ++n) {
        const int buf = n & 1;
        const bool more = n + 1 < S::NB;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const BPlanes<P> ap = src.template planes<P>(u, s, areg);
            __builtin_amdgcn_sched_barrier(0);
            if (s + 1 < S::STEPS) src.load_half(s + 1, u, areg);
            if (u == 1 && more) stg.load(S::blk(a, n + 1));
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                BPlanes<P> bp;
#pragma unroll
                for (int pl = 0; pl < P; ++pl) bp.p[pl] = Bs[buf][((u * 4 + t) * P + pl) * 64 + lane];
                acc[t] = b3_mfma6<P>(ap, bp, acc[t]);
            }
        }
        if (more) stg.store(Bs[buf ^ 1]);
        __syncthreads();
    }
}

// ---- softmax of a point's scores in a tile ----------------------------------------------------------------------------------------------
// The 16 scores of (point pi, the lane's column) are registers 8 pi .. 8 pi + 7 of the two lane halves: the max and the sums are in-lane
// plus ONE v_permlane32_swap each.  fv = the value rows in the same order.
struct AttGSoftmax {
    float e[8];  // exp(s - max) of the lane's eight rows
    float inv;   // 1 / z
    float agg;   // sum_k p F
};
__device__ __forceinline__ AttGSoftmax attg_softmax(const f32x16& acc, int pi, const float (&fv)[8])
{
    AttGSoftmax r;
    float m = acc[8 * pi];
#pragma unroll
    for (int j = 1; j < 8; ++j) m = fmaxf(m, acc[8 * pi + j]);
    m = attg_swap_max(m);
    float z = 0.f, num = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        r.e[j] = __expf(acc[8 * pi + j] - m);
        z += r.e[j];
        num = __builtin_fmaf(r.e[j], fv[j], num);
    }
    z = attg_swap_sum(z);
    num = attg_swap_sum(num);
    r.inv = __builtin_amdgcn_rcpf(z);
    r.agg = num * r.inv;
    return r;
}
// backward on top of it (g = dagg of the point at the lane's column): the direct term pg = p g goes to the point's registers of the dF tile
// `direct` (ADD: on top of what they hold), dS = pg (F - agg) replaces the scores
template <bool ADD>
__device__ __forceinline__ void attg_softmax_bwd(f32x16& acc, f32x16& direct, int pi, const float (&fv)[8], float g)
{
    const AttGSoftmax sm = attg_softmax(acc, pi, fv);
    const float ginv = g * sm.inv;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float pg = sm.e[j] * ginv;
        direct[8 * pi + j] = ADD ? direct[8 * pi + j] + pg : pg;
        acc[8 * pi + j] = pg * (fv[j] - sm.agg);
    }
}

// ---- the transposing product ------------------------------------------------------------------------------------------------------------
// T = X^T . I on the matrix pipe (one MFMA per plane and 16 rows with an identity operand) turns an accumulator tile (lane = column,
// registers = rows) into lane = row, registers = columns: register r of lane (c32, hl) of T = X[row c32][column row0() + attg_acc_row(r)] --
// the layout in which a row leaves as 16-byte stores, and the row operand of the next product register for register (K axis in
// accumulator order: attg_tile_planes of T).

// registers 8 k .. 8 k + 7 of a tile (the lane's eight k-slots of K chunk k in accumulator order) as operand planes
template <int P>
__device__ __forceinline__ BPlanes<P> attg_tile_planes(const f32x16& x, int k)
{
    return b3_split8<P>(make_float4(x[8 * k], x[8 * k + 1], x[8 * k + 2], x[8 * k + 3]), make_float4(x[8 * k + 4], x[8 * k + 5], x[8 * k + 6], x[8 * k + 7]));
}

struct AttGTranspose {
    // k-slot (chunk kap, lane half hl, element j) of an accumulator tile is its row 16 kap + 4 hl + attg_acc_row(j); lane (n = c32, hl) of
    // chunk kap holds 1.0 in the slot whose row is n (one lane half has it)
    uint4 ident[2];
    __device__ __forceinline__ explicit AttGTranspose(const AttGLane& ln)
    {
        const bool mine = ((ln.c32 >> 2) & 1) == ln.hl;
        const int j = (ln.c32 & 3) + 4 * ((ln.c32 >> 3) & 1), kap = ln.c32 >> 4;
        const unsigned one = 0x3F80u << (16 * (j & 1));
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const bool on = mine && kap == k;
            ident[k].x = (on && (j >> 1) == 0) ? one : 0u;
            ident[k].y = (on && (j >> 1) == 1) ? one : 0u;
            ident[k].z = (on && (j >> 1) == 2) ? one : 0u;
            ident[k].w = (on && (j >> 1) == 3) ? one : 0u;
        }
    }
    template <int P>
    __device__ __forceinline__ f32x16 transposed(const f32x16& x) const
    {
        f32x16 T;
#pragma unroll
        for (int r = 0; r < 16; ++r) T[r] = 0.f;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const BPlanes<P> xp = attg_tile_planes<P>(x, k);
#pragma unroll
            for (int pl = P - 1; pl >= 0; --pl) T = b3_mfma(xp.p[pl], ident[k], T);  // (smallest pieces first: every partial sum is exact)
        }
        return T;
    }
};

// ---- the dF tile stores -----------------------------------------------------------------------------------------------------------------
// A tile of dF (lane = column, registers = rows) leaves in accumulator row order.  base = wave-uniform address of the tile's first row,
// col = the lane's column in it, nvalid = rows that exist (0, 16, 32: wave-uniform -- registers 8 half .. are the rows of point `half`),
// accum = read-add instead of overwrite (the reads of a point in flight before its first store).
__device__ __forceinline__ void attg_store_df(float* base, int col, int pitch, int nvalid, bool accum, const f32x16& v, const AttGLane& ln)
{
    float* out = base + (ln.row0() * pitch + col);
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        if (16 * half < nvalid) {
            float old[8];
            if (accum) {
#pragma unroll
                for (int q = 0; q < 8; ++q) old[q] = out[(unsigned)(attg_acc_row(8 * half + q) * pitch)];
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) out[(unsigned)(attg_acc_row(8 * half + q) * pitch)] = accum ? v[8 * half + q] + old[q] : v[8 * half + q];
        }
    }
}
// Rows of bfloat16 (pitch in elements).  A lane owns a column; neighbouring lanes swap every second row (one DPP move each), so the even
// lane holds columns (c, c + 1) of row q and the odd lane those of row q + 1: 4-byte stores of packed pairs (2-byte stores: 1.07 against
// 0.53 ms per launch of attg64_kernel)
__device__ __forceinline__ void attg_store_df(__bf16* base, int col, int pitch, int nvalid, bool accum, const f32x16& v, const AttGLane& ln)
{
    unsigned* b32 = reinterpret_cast<unsigned*>(base + (col & ~1));
    const bool odd = (col & 1) != 0;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        if (16 * half < nvalid) {
            unsigned old[4];
            if (accum) {
#pragma unroll
                for (int q = 0; q < 8; q += 2) old[q >> 1] = b32[(unsigned)((ln.row0() + attg_acc_row(8 * half + q) + (odd ? 1 : 0)) * pitch) >> 1];
            }
#pragma unroll
            for (int q = 0; q < 8; q += 2) {
                const float v0 = v[8 * half + q], v1 = v[8 * half + q + 1];
                const float n0 = __shfl_xor(v0, 1), n1 = __shfl_xor(v1, 1);
                float lo = odd ? n1 : v0, hi = odd ? v1 : n0;  // (row q + odd: columns col & ~1, + 1)
                if (accum) {
                    lo += __uint_as_float(old[q >> 1] << 16);
                    hi += __uint_as_float(old[q >> 1] & 0xffff0000u);
                }
                b32[(unsigned)((ln.row0() + attg_acc_row(8 * half + q) + (odd ? 1 : 0)) * pitch) >> 1] = pack_bf16(lo, hi);
            }
        }
    }
}

}  // namespace ps
