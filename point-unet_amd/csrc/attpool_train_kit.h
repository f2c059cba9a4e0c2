// attpool_train_kit.h -- the pieces of the per-point fused attentive-pooling kernels of the training step (attpool_train.hip), each written
// once: the walk over a wave's points, the K x D tile on its way global -> registers -> LDS -> registers -> global (for the 64 lanes of a
// wave or the 256 of a four-wave group), one description per matrix pipe (LDS layout, weight staging, the three products), the softmax /
// weighted sum / dS step of a column tile, the per-element dF store, and the dWfc epilogues.  Everything is forced inline: the kernels keep
// their own bodies (order of the products, prefetch order, barrier placement).
#pragma once

#include "common.h"
#include "mfma_tile.h"
#include "attpool_train.h"
#include "bf16_io.h"

namespace ps {

// Walks a wave's points (p, p + stride, ...) keeping the cloud of p without a 64-bit division per point (split form: cloud base of fl).
struct PointWalk {
    int p, stride, cloud, rem, n_q;
    __device__ __forceinline__ PointWalk(int first, int stride_, int n_q_) : p(first), stride(stride_), n_q(n_q_ > 0 ? n_q_ : 0x7fffffff)
    {
        cloud = first / n_q;
        rem = first - cloud * n_q;
    }
    __device__ __forceinline__ PointWalk next() const
    {
        PointWalk w = *this;
        w.p += stride;
        w.rem += stride;
        while (w.rem >= n_q) {
            w.rem -= n_q;
            ++w.cloud;
        }
        return w;
    }
};

// The K x D tile of one point as registers of LANES cooperating lanes (64: a wave; 256: the four waves of a group): lane e of pass i holds
// float4 q of row (LANES i + e) / (D/4).  fetch = global -> registers (issued one point AHEAD: a wave works on one point at a time, and at
// two to eight waves per SIMD nothing else covers the latency of these loads); a pipe's commit() = registers -> LDS.  Split form: columns
// [0, D/2) from fl[cloud base + idx[p, row]], [D/2, D) from row p*KN + row of f.
template <int D, int KN, int LANES>
struct TileRegs {
    static constexpr int Q = D / 4, QH = Q / 2, TOT = KN * Q, NV = (TOT + LANES - 1) / LANES;
    float4 v[NV];
    __device__ __forceinline__ void fetch(const AttTrainArgs& a, const PointWalk& w, int lane)
    {
        // wave-uniform 64-bit bases (scalar unit), 32-bit element offsets per lane (a tile spans KN * ld elements; the gathered rows of one
        // cloud n_src * ldl: both far below 2^31 -- checked on the host)
        const float* frow = a.f + (size_t)w.p * KN * a.ld;
        const float* fsrc = a.fl ? a.fl + (size_t)w.cloud * a.n_src * a.ldl : nullptr;
        const int32_t* irow = a.idx ? a.idx + (size_t)w.p * KN : nullptr;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int e = LANES * i + lane;
            if (TOT % LANES == 0 || e < TOT) {
                const unsigned row = (unsigned)e / Q, q = (unsigned)e - row * Q;
                if (!a.fl)
                    v[i] = *reinterpret_cast<const float4*>(frow + (row * (unsigned)a.ld + 4u * q));
                else if (q < (unsigned)QH)
                    v[i] = *reinterpret_cast<const float4*>(fsrc + ((unsigned)irow[row] * (unsigned)a.ldl + 4u * q));
                else if (a.fr_bf16) {  // (the f_xyz half stored as bfloat16: 8 bytes for the four values, kept as loaded -- expand() in front of commit)
                    const uint2 u = *reinterpret_cast<const uint2*>(reinterpret_cast<const unsigned short*>(a.f) + ((size_t)w.p * KN * a.ld + (row * (unsigned)a.ld + 4u * (q - QH))));
                    v[i] = make_float4(__uint_as_float(u.x), __uint_as_float(u.y), 0.f, 0.f);
                }
                else
                    v[i] = *reinterpret_cast<const float4*>(frow + (row * (unsigned)a.ld + 4u * (q - QH)));
            }
        }
    }
    // bfloat16-stored right half -> fp32, where the tile is consumed (converting at fetch would make the wave wait for its own prefetch)
    __device__ __forceinline__ void expand(const AttTrainArgs& a, int lane)
    {
        if (!a.fr_bf16) return;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int e = LANES * i + lane;
            const unsigned q = (unsigned)e % Q;
            if ((TOT % LANES == 0 || e < TOT) && q >= (unsigned)QH) v[i] = unpack_bf16x4(make_uint2(__float_as_uint(v[i].x), __float_as_uint(v[i].y)));
        }
    }
};

// The K x D tile of dF staged in LDS (pitch PA, 8-byte aligned rows) -> global as 16-byte stores: whole rows of df (plain form), or the
// gathered half -> dfl_rows and the f_xyz half -> df (split form).  A point's rows are contiguous in each destination, so the LANES lanes
// write one or two dense spans instead of 4-byte columns of sixteen lanes.  take() reads the staged tile into registers (the LDS tile is
// then free for the next point), put() issues the stores.
template <int D, int KN, int PA, int LANES>
struct RowStore {
    static constexpr int Q = D / 4, QH = Q / 2, TOT = KN * Q, NV = (TOT + LANES - 1) / LANES;
    float4 v[NV];
    __device__ __forceinline__ void take(const float* S, int lane)
    {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int e = LANES * i + lane;
            if (TOT % LANES == 0 || e < TOT) {
                const int row = e / Q, q = e - row * Q;
                const float2 lo = *reinterpret_cast<const float2*>(S + row * PA + 4 * q);
                const float2 hi = *reinterpret_cast<const float2*>(S + row * PA + 4 * q + 2);
                v[i] = make_float4(lo.x, lo.y, hi.x, hi.y);
            }
        }
    }
    __device__ __forceinline__ void put(const AttTrainArgs& a, int64_t p, int lane) const
    {
        float* drow = a.df + (size_t)p * KN * a.lddf;  // (wave-uniform bases, 32-bit lane offsets: as TileRegs::fetch)
        float* lrow = a.dfl_rows ? a.dfl_rows + (size_t)p * KN * a.ld_rows : nullptr;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int e = LANES * i + lane;
            if (TOT % LANES == 0 || e < TOT) {
                const unsigned row = (unsigned)e / Q, q = (unsigned)e - row * Q;
                float4 o = v[i];
                float4* dst;
                if (!a.fl) {
                    dst = reinterpret_cast<float4*>(drow + (row * (unsigned)a.lddf + 4u * q));
                } else if (q < (unsigned)QH && a.fr_bf16) {
                    // (the gathered half's gradient rows, read back once by the gather-reduction, in the same storage format: ld_rows in elements)
                    *reinterpret_cast<uint2*>(reinterpret_cast<unsigned short*>(a.dfl_rows) + ((size_t)p * KN * a.ld_rows + (row * (unsigned)a.ld_rows + 4u * q))) = pack_bf16x4(o);
                    continue;
                } else if (q < (unsigned)QH) {
                    dst = reinterpret_cast<float4*>(lrow + (row * (unsigned)a.ld_rows + 4u * q));
                } else if (a.fr_bf16) {
                    // the f_xyz half's gradient has the format of the f_xyz rows (ps_set_train_act_bf16): bfloat16, lddf in elements; a second
                    // gradient of the same tensor is added to the stored (rounded) value and the sum is rounded again
                    uint2* d16 = reinterpret_cast<uint2*>(reinterpret_cast<unsigned short*>(a.df) + ((size_t)p * KN * a.lddf + (row * (unsigned)a.lddf + 4u * (q - QH))));
                    if (a.df_accum) {
                        const float4 h = unpack_bf16x4(*d16);
                        o.x += h.x; o.y += h.y; o.z += h.z; o.w += h.w;
                    }
                    *d16 = pack_bf16x4(o);
                    continue;
                } else {
                    dst = reinterpret_cast<float4*>(drow + (row * (unsigned)a.lddf + 4u * (q - QH)));
                    if (a.df_accum) {
                        const float4 h = *dst;
                        o.x += h.x; o.y += h.y; o.z += h.z; o.w += h.w;
                    }
                }
                *dst = o;
            }
        }
    }
};

// ---- one description per matrix pipe ---------------------------------------------------------------------------------------------------
// A pipe knows its pitches and its LDS layout -- [weights][tiles of slot 0][tiles of slot 1] ... in floats, a slot being a wave or a group
// of waves that works on one point; the kernels carve `smem` through the constructor and the host sizes the launch from the same constants
// (att_lds_bytes) -- stages the weights, commits a fetched tile, and computes the three products: the score tile(s), dS . Wfc^T and
// F^T . dS.  Common to both: A = the fp32 value tile (pitch PA; the weighted sum uses the unrounded F, and dF is staged in it once it is
// dead), 16 x 16 output tiles in the layout of mfma_tile.h: lane (c16, g) holds rows 4g .. 4g+3 of column c16.

// fp32 operands on v_mfma_f32_16x16x4_f32.  LDS: W [D][PW], backward: W^T [D][PW]; per slot A [KN][PA], backward: dS [KN][PA].
template <int D_>
struct AttF32Pipe {
    static constexpr int D = D_, KN = 16, NT = D / 16;
    static constexpr int PW = D + 16 + (D % 32 == 16 ? 16 : 0);  // weight pitch = 16 (mod 32): conflict-free B-fragment reads
    static constexpr int PA = D + 2;                               // tile pitch = 2 (mod 32): conflict-free A-fragment reads
    static constexpr int weight_floats(bool bwd) { return (bwd ? 2 : 1) * D * PW; }
    static constexpr int tile_floats(bool bwd) { return (bwd ? 2 : 1) * KN * PA; }
    float *W, *WT, *A, *T;  // T = dS: it only ever feeds the two products
    __device__ __forceinline__ AttF32Pipe(float* smem, bool bwd, int slot)
        : W(smem), WT(bwd ? smem + D * PW : nullptr), A(smem + weight_floats(bwd) + slot * tile_floats(bwd)), T(bwd ? A + KN * PA : nullptr)
    {
    }
    // W (row-major [D, D]) and, in the backward, its transpose
    template <int THREADS>
    __device__ __forceinline__ void stage_weights(const float* __restrict__ w) const
    {
        for (int i = threadIdx.x; i < D * D; i += THREADS) {
            const int r = i / D, c = i - r * D;
            const float v = w[i];
            W[r * PW + c] = v;
            if (WT) WT[c * PW + r] = v;
        }
    }
    template <int LANES>
    __device__ __forceinline__ void commit(const TileRegs<D, KN, LANES>& t, int lane) const
    {
        constexpr int Q = D / 4, TOT = KN * Q, RP = LANES / Q;  // (rows per pass: a lane keeps its float4 column)
        const int row0 = lane / Q, q = lane - row0 * Q;
        float* dst0 = A + row0 * PA + 4 * q;
#pragma unroll
        for (int i = 0; i < TileRegs<D, KN, LANES>::NV; ++i) {
            if (TOT % LANES == 0 || LANES * i + lane < TOT) {
                float* dst = dst0 + i * RP * PA;
                dst[0] = t.v[i].x; dst[1] = t.v[i].y; dst[2] = t.v[i].z; dst[3] = t.v[i].w;
            }
        }
    }
    // scores of column tile ct: C[k][c] = sum_j F[k][j] W[j][16 ct + c]
    __device__ __forceinline__ f32x4 score_tile(int ct, int lane) const
    {
        const float* xa = A + (lane & 15) * PA + (lane >> 4);
        const float* wb = W + (lane >> 4) * PW + ct * 16 + (lane & 15);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < D / 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[4 * s], wb[4 * s * PW], acc, 0, 0, 0);
        return acc;
    }
    // all NT column tiles at once, the k steps outermost: NT independent accumulator chains in flight (a tile on its own is a chain of D/4
    // dependent MFMAs), one A-fragment read per k step for all of them, and the softmax VALU work of the tiles follows as one block that
    // the other waves' matrix work can overlap
    __device__ __forceinline__ void score_tiles(int lane, f32x4 (&acc)[NT]) const
    {
        const float* xa = A + (lane & 15) * PA + (lane >> 4);
        const float* wb = W + (lane >> 4) * PW + (lane & 15);
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < D / 4; ++s) {
            const float av = xa[4 * s];
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, wb[4 * s * PW + 16 * t], acc[t], 0, 0, 0);
        }
    }
    __device__ __forceinline__ void store_ds(int row, int col, float v) const { T[row * PA + col] = v; }
    // column tile tj of dS . Wfc^T on top of `acc`
    __device__ __forceinline__ f32x4 df_tile(int tj, int lane, f32x4 acc) const
    {
        const float* xa = T + (lane & 15) * PA + (lane >> 4);
        const float* wb = WT + (lane >> 4) * PW + tj * 16 + (lane & 15);
#pragma unroll
        for (int s = 0; s < D / 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[4 * s], wb[4 * s * PW], acc, 0, 0, 0);
        return acc;
    }
    // dw[ti][t] += (F^T . dS) tile (ti, c0 + t): contraction over the K = 16 rows, four MFMA steps per tile pair
    template <int NC>
    __device__ __forceinline__ void dw_accumulate(f32x4 (&dw)[NT][NC], int c0, int g, int c16) const
    {
#pragma unroll
        for (int s = 0; s < KN / 4; ++s) {
            float fa[NT], db[NC];
#pragma unroll
            for (int t = 0; t < NT; ++t) fa[t] = A[(4 * s + g) * PA + t * 16 + c16];  // A operand: F^T[i = 16 t + c16][k = 4 s + g]
#pragma unroll
            for (int t = 0; t < NC; ++t) db[t] = T[(4 * s + g) * PA + (c0 + t) * 16 + c16];  // B operand: dS[k][j = 16 (c0 + t) + c16]
#pragma unroll
            for (int ti = 0; ti < NT; ++ti)
#pragma unroll
                for (int tj = 0; tj < NC; ++tj) dw[ti][tj] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[ti], db[tj], dw[ti][tj], 0, 0, 0);
        }
    }
};

// bf16 mode (Trainer(mlp_dtype="bf16")) on v_mfma_f32_16x16x16_bf16: the operands of the three products are rounded to bfloat16 (RNE) -- F
// and Wfc for the scores, dS and Wfc^T for the input gradient, F and dS for the weight gradient -- and kept AS bfloat16 in LDS: both weight
// orientations, the tile of F and the tile of dS.  Lane (i, g) supplies k = 4g .. 4g+3, i.e. ONE 8-byte LDS read per operand and sixteen k
// per instruction (D/16 instructions per 16 x 16 output tile instead of D/4); the output layout is that of the fp32 16x16x4 tile, so the
// softmax, the direct term, the stores and the dWfc epilogues are shared.  LDS pitches are 32 bytes (mod 128): the 64 lanes' 8-byte reads
// spread over the banks four to a word, the minimum.
// LDS: backward: Wb [D][PB]; WTb [D][PB] (bfloat16); per slot A [KN][PA] (fp32), Xb [KN][PB], backward: dS [KN][PB] (bfloat16).
typedef short bf16x4s __attribute__((ext_vector_type(4)));

// round to nearest even on v_cvt_pk_bf16_f32 (one instruction per PAIR; the bit-twiddling form was five per element in an issue-bound kernel)
__device__ __forceinline__ unsigned bf16_bits(float x) { return pack_bf16(x, 0.f) & 0xffffu; }

template <int D_>
struct AttBf16Pipe {
    static constexpr int D = D_, KN = 16, NT = D / 16;
    static constexpr int PB = D == 16 ? 16 : (D == 32 ? 48 : (D == 64 ? 80 : 144));  // bfloat16 elements per tile / weight row: 32, 96, 160, 288 bytes
    static constexpr int PA = D + 2;
    static constexpr int weight_floats(bool bwd) { return (bwd ? 2 : 1) * (D * PB / 2); }
    static constexpr int tile_floats(bool bwd) { return KN * PA + (bwd ? 2 : 1) * (KN * PB / 2); }
    unsigned short *Wb, *WTb;  // Wb[i][j] = bf16(W[i][j]) (backward only), WTb[j][i] = bf16(W[i][j])
    float* A;
    unsigned short *Xb, *Tb;  // Tb = dS, rounded: it only ever feeds the two products
    __device__ __forceinline__ AttBf16Pipe(float* smem, bool bwd, int slot)
        : Wb(bwd ? reinterpret_cast<unsigned short*>(smem) : nullptr), WTb(reinterpret_cast<unsigned short*>(smem + (bwd ? D * PB / 2 : 0))),
          A(smem + weight_floats(bwd) + slot * tile_floats(bwd)), Xb(reinterpret_cast<unsigned short*>(A + KN * PA)), Tb(bwd ? Xb + KN * PB : nullptr)
    {
    }
    template <int THREADS>
    __device__ __forceinline__ void stage_weights(const float* __restrict__ w) const
    {
        for (int i = threadIdx.x; i < D * D; i += THREADS) {
            const int r = i / D, c = i - r * D;
            const unsigned short v = (unsigned short)bf16_bits(w[i]);
            if (Wb) Wb[r * PB + c] = v;
            WTb[c * PB + r] = v;
        }
    }
    // a fetched tile -> A (fp32) and Xb (bfloat16)
    template <int LANES>
    __device__ __forceinline__ void commit(const TileRegs<D, KN, LANES>& t, int lane) const
    {
        constexpr int Q = D / 4, TOT = KN * Q, RP = LANES / Q;  // (rows per pass: a lane keeps its float4 column)
        const int row0 = lane / Q, q = lane - row0 * Q;
        float* dst0 = A + row0 * PA + 4 * q;
        unsigned short* xb0 = Xb + row0 * PB + 4 * q;
#pragma unroll
        for (int i = 0; i < TileRegs<D, KN, LANES>::NV; ++i) {
            if (TOT % LANES == 0 || LANES * i + lane < TOT) {
                const float4 v = t.v[i];
                float* dst = dst0 + i * RP * PA;
                dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
                *reinterpret_cast<uint2*>(xb0 + i * RP * PB) = pack_bf16x4(v);
            }
        }
    }
    // acc + C, C[k][c] = sum_j X[k][j] B[j][16 ct + c] with X rows and the B columns both stored k-contiguous: Xs[row][j], Bt[col][j]
    static __device__ __forceinline__ f32x4 tile_mma(const unsigned short* Xs, const unsigned short* Bt, int ct, int lane, f32x4 acc)
    {
        const bf16x4s* xa = reinterpret_cast<const bf16x4s*>(Xs + (lane & 15) * PB + 4 * (lane >> 4));
        const bf16x4s* wb = reinterpret_cast<const bf16x4s*>(Bt + (ct * 16 + (lane & 15)) * PB + 4 * (lane >> 4));
#pragma unroll
        for (int kk = 0; kk < D / 16; ++kk) acc = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(xa[4 * kk], wb[4 * kk], acc, 0, 0, 0);
        return acc;
    }
    __device__ __forceinline__ f32x4 score_tile(int ct, int lane) const { return tile_mma(Xb, WTb, ct, lane, f32x4{0.f, 0.f, 0.f, 0.f}); }
    __device__ __forceinline__ void store_ds(int row, int col, float v) const { Tb[row * PB + col] = (unsigned short)bf16_bits(v); }
    // column tile tj of dS . Wfc^T on top of `acc`: out[row][i] = sum_j dS[row][j] W[i][j]  (B columns = rows of W: Wb)
    __device__ __forceinline__ f32x4 df_tile(int tj, int lane, f32x4 acc) const { return tile_mma(Tb, Wb, tj, lane, acc); }
    // dw[ti][t] += (F^T . dS) tile (ti, c0 + t): ONE 16-row contraction per tile pair (lane (i, g) supplies rows 4g .. 4g+3 of column i)
    template <int NC>
    __device__ __forceinline__ void dw_accumulate(f32x4 (&dw)[NT][NC], int c0, int g, int c16) const
    {
        bf16x4s fa[NT], db[NC];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const unsigned short* xp = Xb + (4 * g) * PB + t * 16 + c16;
            fa[t] = bf16x4s{(short)xp[0], (short)xp[PB], (short)xp[2 * PB], (short)xp[3 * PB]};
        }
#pragma unroll
        for (int t = 0; t < NC; ++t) {
            const unsigned short* tp = Tb + (4 * g) * PB + (c0 + t) * 16 + c16;
            db[t] = bf16x4s{(short)tp[0], (short)tp[PB], (short)tp[2 * PB], (short)tp[3 * PB]};
        }
#pragma unroll
        for (int ti = 0; ti < NT; ++ti)
#pragma unroll
            for (int tj = 0; tj < NC; ++tj) dw[ti][tj] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(fa[ti], db[tj], dw[ti][tj], 0, 0, 0);
    }
};

// (dWfc partials per wave instead of per workgroup when the cross-wave reduction buffer would outgrow LDS)
constexpr bool att_wave_partials(int D, int WAVES) { return (size_t)WAVES * D * D * sizeof(float) > 128 * 1024; }

// Dynamic LDS of a kernel whose `slots` waves or groups each carve a tile set from Pipe; `reduced_waves` > 0: the same buffer later holds
// that many D x D dWfc partials (att_reduce_dw)
template <class Pipe>
constexpr size_t att_lds_bytes(bool bwd, int slots, int reduced_waves)
{
    const size_t tiles = (size_t)Pipe::weight_floats(bwd) + (size_t)slots * Pipe::tile_floats(bwd), red = (size_t)reduced_waves * Pipe::D * Pipe::D;
    return sizeof(float) * (tiles > red ? tiles : red);
}

// ---- the softmax over the 16 rows of column tile ct, the weighted sum, dS ----
struct AttSoftmax {
    float e[4], fv[4], inv, agg;  // this lane's rows 4g .. 4g+3: exp(s - max) and F; 1 / sum over the rows; agg = sum_k p F of the channel
};
template <class Pipe>
__device__ __forceinline__ AttSoftmax att_softmax_tile(const Pipe& P, const f32x4& s, int ct, int g, int c16)
{
    AttSoftmax o;
    float m = fmaxf(fmaxf(s[0], s[1]), fmaxf(s[2], s[3]));
    m = xor_max(m);
    float ssum = 0.f, num = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        o.e[r] = __expf(s[r] - m);
        o.fv[r] = P.A[(4 * g + r) * Pipe::PA + ct * 16 + c16];
        ssum += o.e[r];
        num = __builtin_fmaf(o.e[r], o.fv[r], num);
    }
    ssum = xor_sum(ssum);
    num = xor_sum(num);
    o.inv = __builtin_amdgcn_rcpf(ssum);  // (v_rcp_f32, 1 ulp: the IEEE division is ten instructions in an issue-bound loop)
    o.agg = num * o.inv;
    return o;
}
// backward: dS[k,c] = p g (F - agg) of the tile -> the pipe's dS tile; returns the direct term p g (it seeds dS . Wfc^T)
template <class Pipe>
__device__ __forceinline__ f32x4 att_ds_tile(const Pipe& P, const AttSoftmax& t, float gch, int ct, int g, int c16)
{
    f32x4 dfd;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float pr = t.e[r] * t.inv;
        dfd[r] = pr * gch;
        P.store_ds(4 * g + r, ct * 16 + c16, pr * gch * (t.fv[r] - t.agg));
    }
    return dfd;
}

// dagg of point p for NC column tiles from c0
template <int D, int NC>
__device__ __forceinline__ void att_load_dagg(const AttTrainArgs& a, int64_t p, int c0, int c16, float (&gv)[NC])
{
#pragma unroll
    for (int t = 0; t < NC; ++t) gv[t] = a.dagg[(size_t)p * D + (c0 + t) * 16 + c16];
}

// ---- dF of column `col`, rows 4g .. 4g+3 of point p -> global, element by element (the outputs that cannot take 16-byte row stores) ----
template <int D, int KN>
__device__ __forceinline__ void att_store_df_elems(const AttTrainArgs& a, int64_t p, int g, int col, const f32x4& acc)
{
    const size_t row0 = (size_t)(p * KN + 4 * g);  // the lane's first row of [R*K, .]
    if (!a.fl) {
        float* q = a.df + row0 * a.lddf + col;
#pragma unroll
        for (int r = 0; r < 4; ++r) q[(size_t)r * a.lddf] = acc[r];
    } else if (col >= D / 2 && a.fr_bf16) {  // f_xyz half as bfloat16 rows (the float-atomic scatter form: element by element)
        __bf16* q = reinterpret_cast<__bf16*>(a.df) + row0 * a.lddf + col - D / 2;
#pragma unroll
        for (int r = 0; r < 4; ++r, q += a.lddf) *q = (__bf16)(a.df_accum ? (float)*q + acc[r] : acc[r]);
    } else if (col >= D / 2) {  // f_xyz half: plain rows
        float* q = a.df + row0 * a.lddf + col - D / 2;
#pragma unroll
        for (int r = 0; r < 4; ++r, q += a.lddf) *q = a.df_accum ? *q + acc[r] : acc[r];
    } else if (a.dfl_rows && a.fr_bf16) {
        __bf16* q = reinterpret_cast<__bf16*>(a.dfl_rows) + row0 * a.ld_rows + col;
#pragma unroll
        for (int r = 0; r < 4; ++r) q[(size_t)r * a.ld_rows] = (__bf16)acc[r];
    } else if (a.dfl_rows) {  // gathered half as plain rows: summed per source row by a gather-reduction afterwards
        float* q = a.dfl_rows + row0 * a.ld_rows + col;
#pragma unroll
        for (int r = 0; r < 4; ++r) q[(size_t)r * a.ld_rows] = acc[r];
    } else {  // gathered half: scatter-add onto the source rows
        const int4 nb = *reinterpret_cast<const int4*>(a.idx + row0);
        const int64_t base = (p / a.n_q) * a.n_src;
        atomicAdd(a.dfl + (size_t)(base + nb.x) * a.lddl + col, acc[0]);
        atomicAdd(a.dfl + (size_t)(base + nb.y) * a.lddl + col, acc[1]);
        atomicAdd(a.dfl + (size_t)(base + nb.z) * a.lddl + col, acc[2]);
        atomicAdd(a.dfl + (size_t)(base + nb.w) * a.lddl + col, acc[3]);
    }
}
// column tile tj of dF: staged in the (dead) value tile for the 16-byte row stores, or stored element by element
template <class Pipe>
__device__ __forceinline__ void att_stage_df(const Pipe& P, int tj, int g, int c16, const f32x4& acc)
{
#pragma unroll
    for (int r = 0; r < 4; ++r) P.A[(4 * g + r) * Pipe::PA + tj * 16 + c16] = acc[r];
}
template <class Pipe>
__device__ __forceinline__ void att_put_df(const Pipe& P, const AttTrainArgs& a, int64_t p, int tj, int g, int c16, const f32x4& acc)
{
    if (a.vec_store) att_stage_df(P, tj, g, c16, acc);
    else att_store_df_elems<Pipe::D, Pipe::KN>(a, p, g, tj * 16 + c16, acc);
}

// ---- dWfc epilogues ----
// accumulators dw[ti][t] = tile (ti, c0 + t) -> a row-major D x D image
template <int D, int NC>
__device__ __forceinline__ void att_store_dw(float* dst, const f32x4 (&dw)[D / 16][NC], int c0, int g, int c16)
{
#pragma unroll
    for (int ti = 0; ti < D / 16; ++ti)
#pragma unroll
        for (int t = 0; t < NC; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) dst[(ti * 16 + 4 * g + r) * D + (c0 + t) * 16 + c16] = dw[ti][t][r];
}
// the workgroup's dWfc partial: waves add up through LDS (fixed order), one plain store per element.  `red` = the whole LDS buffer: weights
// and tiles are dead, it holds the WAVES partials (att_lds_bytes sizes it for them)
template <int D, int WAVES>
__device__ __forceinline__ void att_reduce_dw(float* red, const f32x4 (&dw)[D / 16][D / 16], float* dw_part, int wave, int g, int c16)
{
    __syncthreads();
    att_store_dw<D, D / 16>(red + (size_t)wave * D * D, dw, 0, g, c16);
    __syncthreads();
    for (int i = threadIdx.x; i < D * D; i += WAVES * 64) {
        float sum = 0.f;
        for (int w = 0; w < WAVES; ++w) sum += red[(size_t)w * D * D + i];
        dw_part[(size_t)blockIdx.x * D * D + i] = sum;
    }
}

}  // namespace ps
