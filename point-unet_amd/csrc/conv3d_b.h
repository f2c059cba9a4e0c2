// conv3d_b.h -- what conv3d_bf16.hip (the forward and the data gradient) and conv3d_train_bf16.hip (the weight gradient) share: the
// k-contiguous bfloat16 plane tile of the bf16 matrix pipe's convolutions, and the weight gradient's arguments, which conv3d_train.hip
// fills for its fp32 kernel and for conv3d_train_bf16.hip's alike.
#pragma once

#include "b3_ops.h"
#include "saliency.h"

namespace ps {

constexpr int kBKC = 32;  // K chunk: two k-steps of v_mfma_f32_32x32x16_bf16
constexpr int kPW = 20;   // tile pitch in 32-bit words: 32 bfloat16 and 16 bytes (conv3d_bf16.hip explains why it is conflict free)

// x / up for 0 <= x < 2^31 and up >= 2 without a division: the high word of x * (floor(2^32 / up) + 1) is the quotient or one above it (the
// excess is below x / 2^32 < 1/2), which one multiplication tells apart
__device__ __forceinline__ int div_by(int x, unsigned up, unsigned magic)
{
    const unsigned q = __umulhi((unsigned)x, magic);
    return (int)(q - (q * up > (unsigned)x ? 1u : 0u));
}

constexpr int kWSlab = 4096;  // output voxels per workgroup of the weight gradient

struct BwdWeightArgs {
    const float* x;
    const float* x2;
    const float* dy;
    float* part;       // [B * slabs][nrows][cout]
    int r0, nrows;     // the rows this call computes: [r0, r0 + nrows) of the Ktot kernel rows (tap, ci) and the row of ones (the bias) behind them
    int Ktot, slabs, mtiles;
    int B, Ds, Hs, Ws, C1, C2, up, D, H, W, Do, Ho, Wo, cout;
    int kd, kh, kw, stride, dil, pd, ph, pw;
};

// conv3d_train_bf16.hip: the slab partials of PS_PREC_BF16X3 / PS_PREC_BF16 (fills a.mtiles)
void conv3d_bwd_weight_b_launch(hipStream_t sm, BwdWeightArgs& a, int precision);

// Where PS_PREC_BF16X3 runs the split kernels (a form is routed to them only where it was measured faster than the fp32
// kernel by more than the spread between the windows; the accuracy class is the same either way).  Weight gradient: at least 32 output and
// 64 input channels -- with fewer the 32-wide column tile or the short rows leave the six products no work to hide behind.  Data gradient:
// the 16-byte fetch of dy (conv3d_b_vec: C_out a multiple of 4) -- the others are the layers with one or two output channels.
inline bool conv3d_bwd_weight_split_pays(int cin, int cout) { return cout >= 32 && cin >= 64; }

}  // namespace ps
