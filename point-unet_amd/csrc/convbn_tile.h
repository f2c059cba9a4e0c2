// convbn_tile.h -- the tile kit of the recomputed conv + BatchNorm training passes: smallconv_train.hip (c -> c), rectconv_train.hip (widening
// pairs) and, for the workgroup tail and the host plumbing, convbn_rows.hip.  One text of the geometry, the 16-row tile on its way global ->
// registers -> LDS -> registers -> global, the weight staging, the two MFMA loops (tile . weights; x^T . tile over the 16 rows), the per-channel
// constants, the workgroup tail of the partial sums, and the launch arithmetic.  Everything is forced inline: the kernels keep their own
// bodies (prefetch order, wave_lds_sync placement, compile-time switches) and their own waves-per-workgroup choice.
#pragma once

#include "common.h"
#include "bf16_io.h"
#include "mfma_tile.h"

namespace ps {

template <int CI, int CO>
struct ConvGeom {
    static constexpr int CIP = CI < 16 ? 16 : CI, COP = CO < 16 ? 16 : CO;  // channels padded to a tile
    static constexpr int NTI = CIP / 16, NTO = COP / 16;
    static constexpr int PWO = COP + 16 + (COP % 32 == 16 ? 16 : 0);  // pitch of W  [CIP][.]: 16 (mod 32), conflict-free B-fragment reads
    static constexpr int PWI = CIP + 16 + (CIP % 32 == 16 ? 16 : 0);  // pitch of W^T [COP][.]
    static constexpr int PX = CIP + 2, PZ = COP + 2;                  // tile pitches: 2 (mod 32), conflict-free A-fragment reads
};

// W -> LDS [CIP][PWO] and optionally W^T -> [COP][PWI], zero-padded, rounded to bfloat16 when asked
template <int CI, int CO, int THREADS>
__device__ __forceinline__ void stage_w(const float* __restrict__ w, float* W, float* WT, bool bf16)
{
    using G = ConvGeom<CI, CO>;
    for (int i = threadIdx.x; i < G::CIP * G::COP; i += THREADS) {
        const int r = i / G::COP, c = i - r * G::COP;
        float v = (r < CI && c < CO) ? w[r * CO + c] : 0.f;
        if (bf16) v = round_bf16(v);
        W[r * G::PWO + c] = v;
        if (WT) WT[c * G::PWI + r] = v;
    }
}

// 16 rows of a [R, C] tensor starting at row r0 as registers (lane e of pass i: float4 q of row (64 i + e) / (C/4); rows past R are zero).
// fetch = global -> registers, issued one tile AHEAD of its use (a wave works on one tile at a time: nothing else covers the latency),
// commit = registers -> LDS tile (pitch P; padding columns zeroed), take = LDS tile -> registers (8-byte aligned rows), put = 16-byte stores.
template <int C, int P>
struct RowTile {
    static constexpr int Q = C / 4, TOT = 16 * Q, NV = (TOT + 63) / 64;
    float4 v[NV];
    __device__ __forceinline__ void fetch(const float* __restrict__ x, int ldx, int64_t r0, int64_t R, int lane)
    {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int e = 64 * i + lane;
            v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (TOT % 64 == 0 || e < TOT) {
                const int row = e / Q, q = e - row * Q;
                if (r0 + row < R) v[i] = *reinterpret_cast<const float4*>(x + (size_t)r0 * ldx + (unsigned)(row * ldx + 4 * q));  // (wave-uniform base, 32-bit lane offset)
            }
        }
    }
    // the same from / to rows of bfloat16 (8 bytes per lane and pass; converted at the register)
    template <bool B16>
    __device__ __forceinline__ void fetch_any(const float* __restrict__ x, int ldx, int64_t r0, int64_t R, int lane)
    {
        if constexpr (!B16) return fetch(x, ldx, r0, R, lane);
        const unsigned short* xb = reinterpret_cast<const unsigned short*>(x) + (size_t)r0 * ldx;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int e = 64 * i + lane;
            v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (TOT % 64 == 0 || e < TOT) {
                const int row = e / Q, q = e - row * Q;
                if (r0 + row < R) {  // (the raw 8 bytes: converting here would make the wave wait for its own prefetch)
                    const uint2 u = *reinterpret_cast<const uint2*>(xb + (unsigned)(row * ldx + 4 * q));
                    v[i].x = __uint_as_float(u.x);
                    v[i].y = __uint_as_float(u.y);
                }
            }
        }
    }
    // ... expanded to fp32 where the tile is consumed (in front of commit)
    template <bool B16>
    __device__ __forceinline__ void expand()
    {
        if constexpr (B16) {
#pragma unroll
            for (int i = 0; i < NV; ++i) v[i] = unpack_bf16x4(make_uint2(__float_as_uint(v[i].x), __float_as_uint(v[i].y)));
        }
    }
    __device__ __forceinline__ void commit(float* A, int lane, bool bf16 = false) const
    {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int e = 64 * i + lane;
            if (TOT % 64 == 0 || e < TOT) {
                const int row = e / Q, q = e - row * Q;
                float* dst = A + row * P + 4 * q;
                if (bf16) {
                    dst[0] = round_bf16(v[i].x); dst[1] = round_bf16(v[i].y); dst[2] = round_bf16(v[i].z); dst[3] = round_bf16(v[i].w);
                } else {
                    dst[0] = v[i].x; dst[1] = v[i].y; dst[2] = v[i].z; dst[3] = v[i].w;
                }
            }
        }
        if constexpr (C < 16) {  // padding columns (read as operands of the products)
            for (int e = lane; e < 16 * (16 - C); e += 64) A[(e / (16 - C)) * P + C + e % (16 - C)] = 0.f;
        }
    }
    __device__ __forceinline__ void take(const float* S, int lane)
    {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int e = 64 * i + lane;
            if (TOT % 64 == 0 || e < TOT) {
                const int row = e / Q, q = e - row * Q;
                const float2 lo = *reinterpret_cast<const float2*>(S + row * P + 4 * q);
                const float2 hi = *reinterpret_cast<const float2*>(S + row * P + 4 * q + 2);
                v[i] = make_float4(lo.x, lo.y, hi.x, hi.y);
            }
        }
    }
    __device__ __forceinline__ void add(const RowTile& o)
    {
#pragma unroll
        for (int i = 0; i < NV; ++i) { v[i].x += o.v[i].x; v[i].y += o.v[i].y; v[i].z += o.v[i].z; v[i].w += o.v[i].w; }
    }
    __device__ __forceinline__ void lrelu()
    {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            v[i].x = v[i].x < 0.f ? 0.2f * v[i].x : v[i].x; v[i].y = v[i].y < 0.f ? 0.2f * v[i].y : v[i].y;
            v[i].z = v[i].z < 0.f ? 0.2f * v[i].z : v[i].z; v[i].w = v[i].w < 0.f ? 0.2f * v[i].w : v[i].w;
        }
    }
    __device__ __forceinline__ void put(float* __restrict__ out, int ldo, int64_t r0, int64_t R, int lane) const
    {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int e = 64 * i + lane;
            if (TOT % 64 == 0 || e < TOT) {
                const int row = e / Q, q = e - row * Q;
                if (r0 + row < R) *reinterpret_cast<float4*>(out + (size_t)r0 * ldo + (unsigned)(row * ldo + 4 * q)) = v[i];
            }
        }
    }
    template <bool B16>
    __device__ __forceinline__ void put_any(float* __restrict__ out, int ldo, int64_t r0, int64_t R, int lane) const
    {
        if constexpr (!B16) return put(out, ldo, r0, R, lane);
        unsigned short* ob = reinterpret_cast<unsigned short*>(out) + (size_t)r0 * ldo;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int e = 64 * i + lane;
            if (TOT % 64 == 0 || e < TOT) {
                const int row = e / Q, q = e - row * Q;
                if (r0 + row < R) *reinterpret_cast<uint2*>(ob + (unsigned)(row * ldo + 4 * q)) = pack_bf16x4(v[i]);
            }
        }
    }
};

// column tile ct of Y = A . B, A a 16 x K tile (pitch PA) and B [K][.] (pitch PB) in LDS: lane (c16, g) gets rows 4 g + r (r = 0..3) of
// column 16 ct + c16.  y = x . W and dx = dy . W^T of every kernel.
template <int K, int PA, int PB>
__device__ __forceinline__ f32x4 tile_product(const float* A, const float* B, int ct, int lane)
{
    const float* xa = A + (lane & 15) * PA + (lane >> 4);
    const float* wb = B + (lane >> 4) * PB + ct * 16 + (lane & 15);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < K / 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[4 * s], wb[4 * s * PB], acc, 0, 0, 0);
    return acc;
}

// d1 += X^T . B1 (TWO: and d2 += X^T . B2): contraction over the 16 rows of the tiles X (pitch PX) and B (pitch PB), four MFMA steps per
// pair of column tiles.  A operand: x^T[i = 16 t + c16][k = 4 s + g]
template <int NTI, int NTO, int PX, int PB, bool TWO>
__device__ __forceinline__ void xt_mma(const float* X, const float* B1, const float* B2, f32x4 (&d1)[NTI][NTO], f32x4 (&d2)[NTI][NTO], int lane)
{
    const int o = (lane >> 4), c16 = lane & 15;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        float fa[NTI], f1[NTO], f2[NTO];
#pragma unroll
        for (int t = 0; t < NTI; ++t) fa[t] = X[(4 * s + o) * PX + t * 16 + c16];
#pragma unroll
        for (int u = 0; u < NTO; ++u) {
            f1[u] = B1[(4 * s + o) * PB + u * 16 + c16];
            if constexpr (TWO) f2[u] = B2[(4 * s + o) * PB + u * 16 + c16];
        }
#pragma unroll
        for (int t = 0; t < NTI; ++t)
#pragma unroll
            for (int u = 0; u < NTO; ++u) {
                d1[t][u] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[t], f1[u], d1[t][u], 0, 0, 0);
                if constexpr (TWO) d2[t][u] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[t], f2[u], d2[t][u], 0, 0, 0);
            }
    }
}
template <int NTI, int NTO, int PX, int PB>
__device__ __forceinline__ void xt_mma(const float* X, const float* B, f32x4 (&d)[NTI][NTO], int lane)
{
    xt_mma<NTI, NTO, PX, PB, false>(X, B, nullptr, d, d, lane);
}

// per-channel constants of this lane's columns (times mul)
template <int NT>
struct Cols {
    float v[NT];
    __device__ __forceinline__ Cols(const float* p, int c16, int C, float mul = 1.f)
    {
#pragma unroll
        for (int t = 0; t < NT; ++t) v[t] = (t * 16 + c16 < C && p) ? p[t * 16 + c16] * mul : 0.f;
    }
};

// ---- the workgroup's partial sums: each wave lays its values out in its slice r of an LDS buffer [WAVES][nv] ...
// the per-column sums v[t] of array k -> r[k * stride + column]: lanes g = 0..3 hold the same columns, butterfly over g
template <class T, int NT, class... A>
__device__ __forceinline__ void cols_to_lds(T* r, int stride, int lane, const A (&... v)[NT])
{
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const T s[] = {xor_sum_lds(v[t])...};
        if ((lane >> 4) == 0) {
#pragma unroll
            for (int k = 0; k < (int)sizeof...(A); ++k) r[k * stride + t * 16 + (lane & 15)] = s[k];
        }
    }
}
// MFMA accumulators d[t][u] -> the row-major matrix [16 NTI][ld]
template <int NTI, int NTO>
__device__ __forceinline__ void acc_to_lds(const f32x4 (&d)[NTI][NTO], float* r, int ld, int lane)
{
#pragma unroll
    for (int u = 0; u < NTO; ++u)
#pragma unroll
        for (int t = 0; t < NTI; ++t)
#pragma unroll
            for (int q = 0; q < 4; ++q) r[(t * 16 + 4 * (lane >> 4) + q) * ld + u * 16 + (lane & 15)] = d[t][u][q];
}
// ... and the waves add up through LDS in order: one store of the workgroup's partial dst[nv]
template <class T, int WAVES>
__device__ __forceinline__ void wg_merge(const T* red, int nv, T* dst)
{
    __syncthreads();
    for (int i = threadIdx.x; i < nv; i += WAVES * 64) {
        T s = 0;
        for (int w = 0; w < WAVES; ++w) s += red[w * nv + i];
        dst[i] = s;
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
// x, apply's out and the gradient rows dz / dx are stored as bfloat16 (ps_set_train_act_bf16; only with ps_set_train_gemm_bf16)
inline bool convbn_rows_bf16(const ps_context* c) { return c->train_act_bf16 && c->train_bf16; }

inline bool rows_ok(const float* p, int64_t ld, int64_t C) { return p && ld >= C && ld % 4 == 0 && (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// grid of a tile pass: a workgroup per `waves` tiles, at most what 256 CUs hold at this much LDS (up to 4 workgroups each)
inline int convbn_blocks(int64_t R, int waves, size_t smem)
{
    const int64_t tiles = (R + 15) / 16;
    const int per_cu = std::max(1, std::min(4, (int)(160 * 1024 / smem)));
    return (int)std::max<int64_t>(1, std::min<int64_t>((tiles + waves - 1) / waves, 256 * per_cu));
}

// raises the kernel's dynamic-LDS limit where needed, and launches
template <class Args>
inline int convbn_launch(ps_context* c, void (*kern)(Args), int blocks, int threads, size_t smem, const Args& a)
{
    if (smem > 48 * 1024) PS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(threads), smem, c->stream, a);
    return PS_OK;
}

}  // namespace ps
