// gemm32.hip -- dense layers of the deep levels (few rows, wide channels) on v_mfma_f32_32x32x2_f32.
//
//   Y[r, :] = act([X1[g1[r]] | X2[g2[r]]] . W + b)        R = 351 .. 11 250 rows, cin = 128 .. 1 536, cout = 64 .. 1 024
//
// the 1x1 convolutions of encoder levels 2-4 and of the decoder (helper_tf_util.conv2d / conv2d_transpose,
// PointSegment/helper_tf_util.py:115-250; RandLANet.py:130-141, 315-321), inference-mode BatchNorm folded on the host.
// rowgemm_direct (16x16x4 tiles, one B fragment per MFMA from L2) ran these shapes at 13-20 % of the fp32 MFMA peak:
// 16-row tiles re-read every weight once per 16 rows, and a launch was little more than one exposed load-latency chain.
// Here a wave owns a 32-row x (32*CW)-column block: a weight fragment (one 16-byte read of the pack_p32 image, attpool.h)
// feeds four 64-cycle MFMAs over 32 rows, activations are read 16 bytes per lane straight from the row-major input (K taken
// in the order {8q + 4*half + t}, as in attpool32.hip), a ring of chunks is in flight ahead of the MFMAs, and when the
// grid would not fill the chip the waves of a workgroup split the K axis and add their partial blocks through LDS.
// The kernel's frame is shared with gemm32b.hip (gemm32_frame.h, gemm32_frame_body.h); this file holds the fp32 operand policy, the plan
// and the launch.
#include "attpool.h"
#include "gemm32_frame.h"

namespace ps {

#ifdef PS_G32_PD
constexpr int kGemm32Pd = PS_G32_PD;
#else
constexpr int kGemm32Pd = 2;  // (measured, serial cloud, same box: 2 / 3 chunks ahead 1.306-1.308 ms, 4: 1.325, 8: 1.315 -- the K slices are 4-16 chunks)
#endif

// operand policy of the frame (gemm32_frame.h): a chunk is 8 inputs -- one float4 of activations (K taken in the order {8q + 4*half + t}) and one float4 of
// the pack_p32 image per column block, four MFMAs of K = 2.  RW is always 1.
struct Gemm32Fp32 {
    static constexpr int KC = 8, WV = 1;
    using wvec = float4;
    template <int RW, int CW>
    static constexpr int pd() { return kGemm32Pd; }
    template <int RW, int CW>
    static __device__ __forceinline__ void products(const float4 (&x)[RW][1], const float4 (&w)[CW][1], f32x16 (&acc)[RW][CW])
    {
        static_assert(RW == 1, "gemm32: one row block per wave");
#pragma unroll
        for (int j = 0; j < CW; ++j) {
            acc[0][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(x[0][0].x, w[j][0].x, acc[0][j], 0, 0, 0);
            acc[0][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(x[0][0].y, w[j][0].y, acc[0][j], 0, 0, 0);
            acc[0][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(x[0][0].z, w[j][0].z, acc[0][j], 0, 0, 0);
            acc[0][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(x[0][0].w, w[j][0].w, acc[0][j], 0, 0, 0);
        }
    }
};

template <int CW, int SK>
__global__ __launch_bounds__(SK > 4 ? 64 * SK : 256) void gemm32_kernel(Gemm32Args a)
{
    using Op = Gemm32Fp32;
    constexpr int RW = 1;
#include "gemm32_frame_body.h"
}

bool gemm32_fits(const PackedLinear& L, const RowSrc& s1, const RowSrc& s2, int64_t R, int ldy)
{
    return gemm32_fits_kc(L.w32, Gemm32Fp32::KC, L, s1, s2, R, ldy);
}

Gemm32Plan gemm32_plan(const Tuning& tn, int64_t R, int cin, int cout)
{
    Gemm32Plan p;
    const int rblocks = (int)((R + 31) / 32);
    // two column blocks per wave (a row fragment feeds eight MFMAs) once that still leaves a wave for every SIMD
    p.cw = (cout % 64 == 0 && (int64_t)rblocks * (cout / 64) >= 1024) ? 2 : 1;
    p.cgroups = cout / (32 * p.cw);
    // split K across the waves of a workgroup while the plain grid leaves SIMDs idle (1 024 of them) and the slices stay >= 8 chunks
    const int64_t units = (int64_t)rblocks * p.cgroups;
    p.sk = 1;
    while (p.sk < 8 && units * p.sk < 1536 && cin / 8 / (p.sk * 2) >= 8) p.sk *= 2;
    if (p.sk == 8 && tn.gemm32_no_sk8) p.sk = 4;
    const int rb_per_wg = p.sk > 4 ? 1 : 4 / p.sk;
    p.rgroups = (rblocks + rb_per_wg - 1) / rb_per_wg;
    p.rw = 1;
    p.pd = kGemm32Pd;
    return p;
}

int gemm32(ps_context* c, const PackedLinear& L, const RowSrc& s1, const RowSrc& s2, int64_t R, float* y, int ldy)
{
    if (R <= 0) return PS_OK;
    PS_CHECK(gemm32_fits(L, s1, s2, R, ldy), "gemm32: shape / alignment not supported (cin %d, cout %d)", L.cin, L.cout);
    const Gemm32Plan p = gemm32_plan(c->tune, R, L.cin, L.cout);
    const Gemm32Args a = gemm32_args(L.w32, L, s1, s2, R, y, ldy, p);
    const int cw = p.cw, sk = p.sk;
    const dim3 block(sk > 4 ? 64 * sk : 256);
    const unsigned grid = 8u * (unsigned)((a.rgroups * a.cgroups + 7) / 8);
#define PS_G32(CW)                                                                                       \
    if (sk == 1) hipLaunchKernelGGL((gemm32_kernel<CW, 1>), dim3(grid), block, 0, c->stream, a);         \
    else if (sk == 2) hipLaunchKernelGGL((gemm32_kernel<CW, 2>), dim3(grid), block, 0, c->stream, a);    \
    else if (sk == 4) hipLaunchKernelGGL((gemm32_kernel<CW, 4>), dim3(grid), block, 0, c->stream, a);    \
    else hipLaunchKernelGGL((gemm32_kernel<CW, 8>), dim3(grid), block, 0, c->stream, a)
    if (cw == 2) { PS_G32(2); } else { PS_G32(1); }
#undef PS_G32
    PS_HIP(hipGetLastError());
    return PS_OK;
}

}  // namespace ps
