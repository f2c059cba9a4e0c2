// conv3d_kit.h -- what the 3-D convolution's kernels share: conv3d.hip (the fp32 forward and data gradient),
// conv3d_bf16.hip (the same two on the bf16 matrix pipe), conv3d_train.hip (the entries of the gradients and the fp32 weight gradient) and
// conv3d_train_bf16.hip (the weight gradient on the bf16 pipe).  Every rule stands here once: the entries' geometry check, which form a
// launcher takes, the rows of the forward and the data gradient, the division-free / up, the weight gradient's arguments, the fp32 chunk
// product with its rounding chain -- a chunk of 32 k is summed in a fresh accumulator and then added to the running one -- and the bf16
// pipe's B-tile staging and C-row map.  What is NOT here, because behind a call the kernels compile to other instructions than before and
// measured slower: the tap's bounds test, the bf16 pipe's chunk product, the weight gradient's row decode, corner table
// and fetch stay written out in their kernels.
#pragma once

#include <type_traits>

#include "b3_ops.h"
#include "mfma_tile.h"
#include "saliency.h"

namespace ps {

// ---- the entries' argument check ---------------------------------------------------------------------------------------------------------------

inline int conv_geometry_ok(const char* who, int64_t B, int64_t Ds, int64_t Hs, int64_t Ws, int64_t C1, int64_t C2, int32_t up, int32_t kd, int32_t kh,
                            int32_t kw, int64_t C_out, int32_t stride, int32_t dilation)
{
    const int64_t lim = 1ll << 31;
    auto kext = [](int k) { return k == 1 || k == 3 || k == 9; };
    PS_CHECK(kext(kd) && kext(kh) && kext(kw), "%s: kernel %d x %d x %d, every extent must be 1, 3 or 9", who, (int)kd, (int)kh, (int)kw);
    PS_CHECK(stride == 1 || stride == 2, "%s: stride = %d, must be 1 or 2", who, (int)stride);
    PS_CHECK(dilation == 1 || dilation == 3 || dilation == 5 || dilation == 7, "%s: dilation = %d, must be 1, 3, 5 or 7", who, (int)dilation);
    PS_CHECK(up >= 1 && up <= 8, "%s: up = %d, must be in [1, 8]", who, (int)up);
    PS_CHECK(B >= 1 && B <= 65535, "%s: B = %lld, must be in [1, 65535]", who, (long long)B);
    PS_CHECK(C1 >= 1 && C2 >= 0 && C1 + C2 <= 384, "%s: C1 = %lld, C2 = %lld (C1 >= 1, C2 >= 0, C1 + C2 <= 384)", who, (long long)C1, (long long)C2);
    PS_CHECK(C_out >= 1 && C_out <= 256, "%s: C_out = %lld, must be in [1, 256]", who, (long long)C_out);
    PS_CHECK(Ds >= 1 && Hs >= 1 && Ws >= 1 && Ds < lim && Hs < lim && Ws < lim && Ds * up * Hs * up < lim && Ds * up * Hs * up * Ws * up < lim
                 && Ds * Hs * Ws * (C1 > C2 ? C1 : C2) < lim && Ds * up * Hs * up * Ws * up * C_out < lim,
             "%s: input %lld x %lld x %lld (every extent >= 1, every tensor below 2^31 elements per sample)", who, (long long)Ds, (long long)Hs,
             (long long)Ws);
    return PS_OK;
}

// ---- which form --------------------------------------------------------------------------------------------------------------------------------

// A launcher's form is (RT, NT): 64 * RT rows and NT column tiles per workgroup.  `tall` picks 128 rows: the forward and the data gradient
// where the rows (output voxels; the virtual input's) are at least 2048, enough to fill the device with such workgroups; the weight gradient
// where it has more than 64 rows.  The column tiles are the fewest that hold `cols` up to 64.  f(RT, NT) gets them as integral constants.
template <int V>
using Int = std::integral_constant<int, V>;

// fp32: 16-wide column tiles, 1, 2 or 4 of them (C_out = 1 and 2 -- the attention's second convolutions and `final` -- run the one-tile form:
// their K is 288 and 3 456, the matrix pipe's empty columns cost less than a millisecond of the full patch)
template <class F>
void conv_form(bool tall, int cols, F&& f)
{
    if (cols <= 16) tall ? f(Int<2>{}, Int<1>{}) : f(Int<1>{}, Int<1>{});
    else if (cols <= 32) tall ? f(Int<2>{}, Int<2>{}) : f(Int<1>{}, Int<2>{});
    else tall ? f(Int<2>{}, Int<4>{}) : f(Int<1>{}, Int<4>{});
}

// bf16 pipe: 32-wide column tiles, 1 or 2 (up to 16 columns leave half a tile empty, as the fp32 tile does at 1 and 2).  SHORT = false: the
// caller has no 64-row forms
template <bool SHORT = true, class F>
void conv_form_b(bool tall, int cols, F&& f)
{
    if constexpr (SHORT) {
        if (!tall) return cols <= 32 ? f(Int<1>{}, Int<1>{}) : f(Int<1>{}, Int<2>{});
    }
    cols <= 32 ? f(Int<2>{}, Int<1>{}) : f(Int<2>{}, Int<2>{});
}

// ---- the rows of the forward and the data gradient -------------------------------------------------------------------------------------------

// Row v of Vo = Do * Ho * Wo as the kernels' fetch wants it, (z, y, x, whether the row exists); all 0 behind the last row.  Forward: the input
// corner of the row's receptive field, o * stride - pad, to which the fetch adds tap * dilation.  GRAD, the data gradient's gather: the row's
// voxel + pad, from which the fetch subtracts tap * dilation and keeps the term where the difference is a whole multiple of the stride.
template <bool GRAD>
__device__ __forceinline__ int4 conv_row(const Conv3dArgs& a, int v, int Vo)
{
    if (v >= Vo) return {0, 0, 0, 0};
    const int ow = v % a.Wo, oh = v / a.Wo % a.Ho, od = v / (a.Wo * a.Ho);
    if constexpr (GRAD) return {od + a.pd, oh + a.ph, ow + a.pw, 1};
    else return {od * a.stride - a.pd, oh * a.stride - a.ph, ow * a.stride - a.pw, 1};
}

// x / up for 0 <= x < 2^31 and up >= 2 without a division: the high word of x * (floor(2^32 / up) + 1) is the quotient or one above it (the
// excess is below x / 2^32 < 1/2), which one multiplication tells apart
__device__ __forceinline__ unsigned div_magic(int up) { return (unsigned)((1ull << 32) / (unsigned)up) + 1u; }
__device__ __forceinline__ int div_by(int x, unsigned up, unsigned magic)
{
    const unsigned q = __umulhi((unsigned)x, magic);
    return (int)(q - (q * up > (unsigned)x ? 1u : 0u));
}

// ---- the weight gradient (fp32: conv3d_train.hip, bf16 pipe: conv3d_train_bf16.hip) ------------------------------------------------------------

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

// ---- fp32: v_mfma_f32_16x16x4_f32 --------------------------------------------------------------------------------------------------------------

constexpr int kKC = 32;        // K chunk
constexpr int kAP = kKC + 2;   // row-major A tile pitch: 2 (mod 32) floats, the A-fragment read is conflict free (mfma_tile.h)
constexpr int kBP = 80;        // k-major tile pitch for up to 64 columns: the four k rows of a fragment read start 16 banks apart

// One K chunk of a wave's RT x NT tiles: the chunk's 8 k-steps in a fresh accumulator, then added to the running one.
// a0: this lane's A element of row tile 0, k-step 0 (row tiles a_rt floats apart, k-steps a_s); b0: the same in the k-major B tile.
template <int RT, int NT>
__device__ __forceinline__ void chunk_mma(const float* a0, int a_rt, int a_s, const float* b0, f32x4 (&acc)[RT][NT])
{
    f32x4 part[RT][NT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int j = 0; j < NT; ++j) part[rt][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < kKC / 4; ++s) {
        float av[RT], bv[NT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) av[rt] = a0[rt * a_rt + s * a_s];
#pragma unroll
        for (int j = 0; j < NT; ++j) bv[j] = b0[s * 4 * kBP + j * 16];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int j = 0; j < NT; ++j) part[rt][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[rt], bv[j], part[rt][j], 0, 0, 0);
    }
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[rt][j] += part[rt][j];
}

// ---- bf16 pipe: v_mfma_f32_32x32x16_bf16 on k-contiguous bfloat16 plane tiles (conv3d_bf16.hip explains the layout) ------------------------------

constexpr int kBKC = 32;  // K chunk: two k-steps of v_mfma_f32_32x32x16_bf16
constexpr int kPW = 20;   // tile pitch in 32-bit words: 32 bfloat16 and 16 bytes (conv3d_bf16.hip explains why it is conflict free)

// Splits or rounds a thread's BK (4 or 8) consecutive k of one B column and stores them to its place in the P planes (ldp words apart)
template <int P, int BK>
__device__ __forceinline__ void stage_b(const float (&breg)[BK], unsigned* dst, int ldp)
{
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = i < BK ? breg[i < BK ? i : 0] : 0.f;
    const BPlanes<P> p = b3_split8<P>(v);
#pragma unroll
    for (int pl = 0; pl < P; ++pl) {
        if constexpr (BK == 8) *reinterpret_cast<uint4*>(dst + pl * ldp) = p.p[pl];
        else *reinterpret_cast<uint2*>(dst + pl * ldp) = make_uint2(p.p[pl].x, p.p[pl].y);
    }
}

// C[m][n] of the 32 x 32 tile: lane (n = lane % 32, hl = lane / 32), register r holds row (r & 3) + 8 (r >> 2) + 4 hl of the tile, whose
// first row is `first`
__device__ __forceinline__ int c_row_b(int first, int r, int hl) { return first + (r & 3) + 8 * (r >> 2) + 4 * hl; }

}  // namespace ps
