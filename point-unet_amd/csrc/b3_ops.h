// b3_ops.h -- operand helpers of the split-bf16 ("bf16x3") matrix products, the one definition that gemm_b3.hip, attpool_gemm.hip,
// gemm32b.hip and attpool32b.hip share (device: split, planes, MFMA; host: b3_piece_of for the weight images):
// v_mfma_f32_32x32x16_bf16 over exact three-way bfloat16 splits of fp32 operands (P = 3: six piece products per fp32 product, fp32
// accumulate, fp32-level error -- attpool32b.hip explains the split) or over ONE plane of round-to-nearest-even bfloat16 (P = 1: the
// bf16-MLP mode of the training step).
//
// Fragment maps of the instruction (wave64, hl = lane >> 5, c32 = lane & 31):
//   A[m][k]: lane (m = c32, hl) holds k = 8 hl + j, j = 0..7      B[k][n]: lane (n = c32, hl) holds k = 8 hl + j
//   C[m][n]: lane (n = c32, hl), register r holds m = (r & 3) + 8 (r >> 2) + 4 hl
#pragma once

#include <hip/hip_runtime.h>

#include "common.h"
#include "mfma_tile.h"

namespace ps {

__device__ __forceinline__ void b3_split_pair(float x, float y, unsigned& q1, unsigned& q2, unsigned& q3)
{
    const unsigned xu = __float_as_uint(x), yu = __float_as_uint(y);
    const float xr = x - __uint_as_float(xu & 0xffff0000u), yr = y - __uint_as_float(yu & 0xffff0000u);  // exact
    const unsigned xru = __float_as_uint(xr), yru = __float_as_uint(yr);
    const float x3 = xr - __uint_as_float(xru & 0xffff0000u), y3 = yr - __uint_as_float(yru & 0xffff0000u);  // exact, 8 bits
    q1 = __builtin_amdgcn_perm(yu, xu, 0x07060302u);  // [y.hi16 : x.hi16]
    q2 = __builtin_amdgcn_perm(yru, xru, 0x07060302u);
    q3 = __builtin_amdgcn_perm(__float_as_uint(y3), __float_as_uint(x3), 0x07060302u);
}
// P = 3: the exact three-way split (fp32 products on the bf16 pipe).  P = 1: ONE plane of round-to-nearest-even bfloat16 -- the bf16-MLP
// mode of the training step (operands rounded to bfloat16, fp32 accumulation), which so runs its large products through the same tiling
// with a sixth of the matrix work: HBM bound ([360k, 256] x [256, 256]: 0.63 ms in rowgemm_direct_bf16 before).
// plane word t = pieces of (x[2t], x[2t+1]), low half = the even element
template <int P>
struct BPlanes {
    uint4 p[P];
};
typedef BPlanes<3> B3Planes;
typedef __bf16 b3_bf16x2 __attribute__((ext_vector_type(2)));
typedef float b3_f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned b3_rne_pair(float a, float b)  // (low half = a: v_cvt_pk_bf16_f32)
{
    return __builtin_bit_cast(unsigned, __builtin_convertvector(b3_f32x2{a, b}, b3_bf16x2));
}
template <int P>
__device__ __forceinline__ BPlanes<P> b3_split8(const float4& lo, const float4& hi)
{
    BPlanes<P> r;
    if constexpr (P == 3) {
        b3_split_pair(lo.x, lo.y, r.p[0].x, r.p[1].x, r.p[2].x);
        b3_split_pair(lo.z, lo.w, r.p[0].y, r.p[1].y, r.p[2].y);
        b3_split_pair(hi.x, hi.y, r.p[0].z, r.p[1].z, r.p[2].z);
        b3_split_pair(hi.z, hi.w, r.p[0].w, r.p[1].w, r.p[2].w);
    } else {
        r.p[0].x = b3_rne_pair(lo.x, lo.y);
        r.p[0].y = b3_rne_pair(lo.z, lo.w);
        r.p[0].z = b3_rne_pair(hi.x, hi.y);
        r.p[0].w = b3_rne_pair(hi.z, hi.w);
    }
    return r;
}
template <int P>
__device__ __forceinline__ BPlanes<P> b3_split8(const float (&x)[8])
{
    return b3_split8<P>(make_float4(x[0], x[1], x[2], x[3]), make_float4(x[4], x[5], x[6], x[7]));
}
__device__ __forceinline__ f32x16 b3_mfma(const uint4& a, const uint4& b, f32x16 acc)
{
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), acc, 0, 0, 0);
}
// the six kept piece products, smallest first
template <int P>
__device__ __forceinline__ f32x16 b3_mfma6(const BPlanes<P>& a, const BPlanes<P>& b, f32x16 acc)
{
    if constexpr (P == 3) {
        acc = b3_mfma(a.p[2], b.p[0], acc);
        acc = b3_mfma(a.p[0], b.p[2], acc);
        acc = b3_mfma(a.p[1], b.p[1], acc);
        acc = b3_mfma(a.p[1], b.p[0], acc);
        acc = b3_mfma(a.p[0], b.p[1], acc);
        acc = b3_mfma(a.p[0], b.p[0], acc);
    } else {
        acc = b3_mfma(a.p[0], b.p[0], acc);
    }
    return acc;
}

// The same on v_mfma_f32_16x16x32_bf16 (regchain.hip): A[m][k]: lane (m = lane & 15, g = lane >> 4) holds k = 8 g + j, j = 0..7;
// B[k][n]: lane (n = lane & 15, g) holds k = 8 g + j; C[m][n]: lane (n, g), register q holds m = 4 g + q -- the C layout of 16x16x4.
// The eight k values of a lane are the two float4 a lane of that C layout holds of two adjacent 16-channel tiles: b3_split8(lo, hi).
__device__ __forceinline__ f32x4 b3_mfma16(const uint4& a, const uint4& b, f32x4 acc)
{
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), acc, 0, 0, 0);
}
__device__ __forceinline__ f32x4 b3_mfma16_6(const BPlanes<1>& a, const BPlanes<1>& b, f32x4 acc)  // one plane: the one product
{
    return b3_mfma16(a.p[0], b.p[0], acc);
}
__device__ __forceinline__ f32x4 b3_mfma16_6(const B3Planes& a, const B3Planes& b, f32x4 acc)  // the six kept piece products, smallest first
{
    acc = b3_mfma16(a.p[2], b.p[0], acc);
    acc = b3_mfma16(a.p[0], b.p[2], acc);
    acc = b3_mfma16(a.p[1], b.p[1], acc);
    acc = b3_mfma16(a.p[1], b.p[0], acc);
    acc = b3_mfma16(a.p[0], b.p[1], acc);
    acc = b3_mfma16(a.p[0], b.p[0], acc);
    return acc;
}

// Host: bfloat16 piece `plane` (0..2) of w, the same split as b3_split_pair, for the weight images packed on the host (pack_p32b,
// pack_b3, pack_b3_locse).  The volatiles are load-bearing: do not remove them.
inline uint16_t b3_piece_of(float w, int plane)
{
    auto trunc16 = [](float x) {
        uint32_t u;
        __builtin_memcpy(&u, &x, 4);
        u &= 0xffff0000u;
        float r;
        __builtin_memcpy(&r, &u, 4);
        return r;
    };
    volatile float w1 = trunc16(w);
    volatile float r1 = w - w1;
    volatile float w2 = trunc16(r1);
    volatile float w3 = r1 - w2;
    const float pick = plane == 0 ? w1 : (plane == 1 ? w2 : w3);
    uint32_t u;
    __builtin_memcpy(&u, &pick, 4);
    return (uint16_t)(u >> 16);
}

// Host: w rounded ONCE to bfloat16, round to nearest even (ties to even) -- what b3_rne_pair / v_cvt_pk_bf16_f32 give for a finite w: the
// one plane of the P = 1 weight images packed on the host (pack_p32b, pack_b3 with planes = 1), and the same value as an fp32
inline uint16_t b3_rne_of(float w)
{
    uint32_t u;
    __builtin_memcpy(&u, &w, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);  // NaN stays NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
inline float b3_rounded(float w)
{
    const uint32_t u = (uint32_t)b3_rne_of(w) << 16;
    float r;
    __builtin_memcpy(&r, &u, 4);
    return r;
}
// piece `plane` of w in an image of `planes` planes (3: the exact split, 1: the rounded value)
inline uint16_t b3_plane_of(float w, int plane, int planes) { return planes == 1 ? b3_rne_of(w) : b3_piece_of(w, plane); }

// the element function of gemm_b3_pack_kernel for the batched form (PackCache): thread i of job j.
// KMAP: the K axis in the order in which a 32x32 accumulator tile hands its values on as the next product's operand (b3_ops.h:
// k-slot (chunk q, lane half hl, element e) = index 32 (q >> 1) + 16 (q & 1) + 8 (e >> 2) + 4 hl + (e & 3)) -- the image of
// attpool_gemm.hip's second product, whose row operand is the transposed accumulator tile of dS.
template <int P, bool KMAP>
__device__ __forceinline__ void b3_pack_elem(const PackJob& j, int64_t i)
{
    const int ncb = j.cout / 32;
    const int lane = (int)(i & 63), cb = (int)((i >> 6) % ncb), q = (int)((i >> 6) / ncb);
    const int hl = lane >> 5;
    const float* src = j.w + (int64_t)(32 * cb + (lane & 31)) * j.sn;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int k = KMAP ? 32 * (q >> 1) + 16 * (q & 1) + 8 * (e >> 2) + 4 * hl + (e & 3) : 16 * q + 8 * hl + e;
        v[e] = src[(int64_t)k * j.sk];
    }
    const BPlanes<P> p = b3_split8<P>(make_float4(v[0], v[1], v[2], v[3]), make_float4(v[4], v[5], v[6], v[7]));
    uint4* dst = static_cast<uint4*>(j.out) + ((size_t)(q * ncb + cb) * P) * 64 + lane;
#pragma unroll
    for (int pl = 0; pl < P; ++pl) dst[64 * pl] = p.p[pl];
}
__device__ __forceinline__ void b3_pack_elem_any(const PackJob& j, int64_t i)
{
    if (j.kind == 3) b3_pack_elem<3, false>(j, i);
    else if (j.kind == 4) b3_pack_elem<1, false>(j, i);
    else if (j.kind == 5) b3_pack_elem<3, true>(j, i);
    else b3_pack_elem<1, true>(j, i);
}

}  // namespace ps
