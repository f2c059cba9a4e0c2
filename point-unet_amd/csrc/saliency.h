// saliency.h -- what conv3d.hip and saliency.hip share: the implicit-GEMM 3-D convolution with its strided forms (the network writes
// every concat part straight into the concat's buffer, so a tensor has a channel pitch), include/pointseg_saliency.h.
#pragma once

#include "../../include/pointseg_saliency_precision.h"
#include "common.h"

namespace ps {

// One convolution.  The input is the channel concat of x (C1 channels, pitch ldx) and x2 (C2, pitch ldx2; nullptr with C2 == 0) at
// [B, Ds, Hs, Ws], up-sampled `up` times by repetition; the output voxel row has pitch ldy.  w: [taps][C1 + C2][cout], w_bstride floats
// further for each sample (0: one kernel for all -- the channel attention folds its per-sample scale into C345_conv's kernel).
struct Conv3dArgs {
    const float* x;
    const float* x2;
    const float* w;
    const float* bias;
    float* y;
    int B, Ds, Hs, Ws, C1, C2, ldx, ldx2, up;
    int kd, kh, kw, cout, stride, dil, ldy;
    int64_t w_bstride;
    int precision;  // PS_PREC_*: 0 (what `= {}` leaves) is the fp32 kernel of conv3d.hip, the others run conv3d_bf16.hip's
    // derived by conv3d_plan
    int D, H, W, Do, Ho, Wo, pd, ph, pw;
    // The data-gradient form of both kernels (grad != 0; conv3d_train.hip fills it, include/pointseg_saliency_train.h): the same implicit
    // GEMM with the roles turned.  x is dy ([B, D, H, W, C1], C2 = 0, up = 1: D, H, W the convolution's OUTPUT extents), the
    // rows are the Do * Ho * Wo voxels i of the convolution's virtual INPUT, the fetch gathers dy[(i + pad - tap * dil) / stride] where that
    // is whole and inside, w is the transposed kernel [taps * C1][ldw] (its first column the first computed channel), cout the computed
    // channels; those below nsplit go to y (pitch ldy), the others to y2 (pitch ldy2).  No bias.
    int grad, ldw, nsplit, ldy2;
    float* y2;
};

inline int same_out(int in, int stride) { return (in + stride - 1) / stride; }
inline int same_pad_before(int in, int k, int stride, int dil)
{
    const int total = (same_out(in, stride) - 1) * stride + (k - 1) * dil + 1 - in;
    return (total > 0 ? total : 0) / 2;
}

void conv3d_plan(Conv3dArgs& a);                   // fills the derived fields
void conv3d_launch(hipStream_t sm, const Conv3dArgs& a);  // (a planned; every limit checked by the caller)
void conv3d_b_launch(hipStream_t sm, const Conv3dArgs& a);  // conv3d_bf16.hip: what conv3d_launch calls for PS_PREC_BF16X3 and PS_PREC_BF16
bool conv3d_b_vec(const Conv3dArgs& a);                     // whether conv3d_b_launch takes the 16-byte activation fetch

inline bool precision_ok(int32_t p) { return p == PS_PREC_FP32 || p == PS_PREC_BF16X3 || p == PS_PREC_BF16; }
// the check of every entry that takes one precision
inline int precision_check(const char* who, int32_t precision)
{
    PS_CHECK(precision_ok(precision), "%s: precision = %d, must be PS_PREC_FP32 (0), PS_PREC_BF16X3 (1) or PS_PREC_BF16 (2)", who, (int)precision);
    return PS_OK;
}

}  // namespace ps
