// gemm32b.hip -- gemm32.hip's dense layers on v_mfma_f32_32x32x16_bf16 over EXACT three-way bfloat16 splits of both fp32 operands
// ("bf16x3", attpool32b.hip: x = x1 + x2 + x3 with 8 significant bits each, six piece products kept, fp32 accumulate -- fp32-level
// error, 2.7 x less matrix-pipe time than the fp32 MFMA, which runs at 1/16 of the bf16 rate on gfx950).
//
//   Y[r, :] = act([X1[g1[r]] | X2[g2[r]]] . W + b)
//
// the 1x1 convolutions of encoder levels 2-4 and of the decoder (helper_tf_util.conv2d / conv2d_transpose,
// PointSegment/helper_tf_util.py:115-250; RandLANet.py:130-141, 315-321) whose product is large enough to be bound by the matrix
// pipe: [mlp2 ; shortcut] of levels 2-4 (1.47 GFLOP each), decoder_0 and the first decoder steps (0.7-1.1 GFLOP).  On the fp32 MFMA
// (gemm32.hip) those seven launches took 24-35 us each, 23 % of the fp32 peak; here 12-24 us (round 4, rocprofv3 kernel trace: decoder_0 28 -> 22,
// first decoder step 35 -> 26 us by hipEvent pairs).  What bounds them now is not the matrix pipe (13 % busy, SQ_VALU_MFMA_BUSY_CYCLES) but
// the grid: 176-704 workgroups of four waves leave one or two waves per SIMD, so a wave's own sequence -- split (56 VALU instructions
// per 16-wide K chunk), twelve MFMAs, the wait for the next chunk -- is exposed end to end, and 352 workgroups on 256 CUs run as 1 + 1.
//
// A wave owns (32 RW) rows x (32 CW) columns: activations are read 32 bytes per lane straight from the row-major input (row = lane & 31,
// eight consecutive K values per lane half: exactly the operand layout of the instruction) and split in registers; the weights come
// pre-split from the layer's three-plane image (pack_p32b: [column block][K chunk of 16][plane][lane] x 16 bytes).  One split of an
// activation fragment feeds CW column blocks, one weight fragment RW row blocks.  When the grid would not fill the chip the four waves of
// a workgroup split the K axis and add their partial blocks through LDS (fixed order).
// The kernel's frame is shared with gemm32.hip (gemm32_frame.h, gemm32_frame_body.h) and the split itself with the other bf16x3 kernels
// (b3_ops.h); this file holds the split operand policy, pack_p32b, the plan and the launch.
#include "attpool.h"
#include "b3_ops.h"
#include "gemm32_frame.h"

namespace ps {

namespace {

// ... for a whole RW x CW block of accumulators, piece product by piece product: consecutive MFMAs go to DIFFERENT accumulators.  Issued
// accumulator by accumulator (six dependent instructions in a row) a wave spent 55 % of its cycles in issue stalls (SQ_WAIT_INST_ANY,
// round 4 counters): a dependent MFMA waits for its predecessor's last pass, and with one wave per SIMD nothing else fills the gap.
template <int P, int RW, int CW>
__device__ __forceinline__ void mfma6_all(const BPlanes<P> (&A)[RW], const BPlanes<P> (&B)[CW], f32x16 (&acc)[RW][CW])
{
    if constexpr (P == 3) {
        constexpr int pa[6] = {2, 0, 1, 1, 0, 0}, pb[6] = {0, 2, 1, 0, 1, 0};  // smallest products first
#pragma unroll
        for (int t = 0; t < 6; ++t)
#pragma unroll
            for (int i = 0; i < RW; ++i)
#pragma unroll
                for (int j = 0; j < CW; ++j) acc[i][j] = b3_mfma(A[i].p[pa[t]], B[j].p[pb[t]], acc[i][j]);
    } else {  // one plane of rounded operands: the one product
#pragma unroll
        for (int i = 0; i < RW; ++i)
#pragma unroll
            for (int j = 0; j < CW; ++j) acc[i][j] = b3_mfma(A[i].p[0], B[j].p[0], acc[i][j]);
    }
}

// PD chunks ahead: a wave's loop is a chain of dependent round trips to L2 / MALL (the weight planes of a layer are read once per 32-row
// block), and one chunk in flight left the launch latency-bound (23 us for 0.74 GFLOP); the ring is refilled in place behind its last reader.
// Round 6, serial cloud on one box: 2 chunks ahead 1.280-1.286 ms, 3: 1.283-1.296, 4 (rounds 4-5): 1.295-1.306; 6 / 8 take 256 VGPRs and run
// the enc2-4 dense stages 0.086 / 0.097 / 0.086 and 0.090 / 0.102 / 0.090 ms against 0.078 / 0.077 / 0.075 -- the K slices of these launches
// are 8-24 chunks, and every chunk fetched past the end of a slice is a wasted request
constexpr int gemm32b_pd(int rw, int cw)
{
#ifdef PS_G32B_PD
    return rw * cw >= 4 ? 3 : PS_G32B_PD;  // (experiment: ring depth of the (1, 1) / (1, 2) tiles)
#else
    return rw * cw >= 4 ? 3 : 2;
#endif
}

// One plane (P = 1: both operands rounded once to bfloat16, PS_PREC_BF16): a chunk is 16 weights of 2 bytes and ONE 32-cycle MFMA per block where
// the split form has six behind 56 VALU instructions, so a chunk's products end ~6 x sooner while the round trip to L2 stays what it is: the
// ring has to hold more chunks to cover the same latency.  Four for every tile shape: (2, 2) then keeps 4 x (16 + 8) = 96 registers of ring
// next to its 64 accumulators, and the K slices of the network's layers (8-24 chunks) are multiples of four.  Reasoned, not measured.
constexpr int gemm32b1_pd() { return 4; }

// operand policy of the frame (gemm32_frame.h): a chunk is 16 inputs -- two float4 of activations per row block (row = lane & 31, eight
// consecutive K values per lane half: exactly the operand layout of the instruction), split in registers, and the P pre-split planes
// of the pack_p32b image per column block; six MFMAs (P = 3) or one (P = 1) of K = 16 per 32 x 32 block.
template <int P>
struct Gemm32Planes {
    static constexpr int KC = 16, WV = P;
    using wvec = uint4;
    template <int RW, int CW>
    static constexpr int pd() { return P == 3 ? gemm32b_pd(RW, CW) : gemm32b1_pd(); }
    template <int RW, int CW>
    static __device__ __forceinline__ void products(const float4 (&x)[RW][2], const uint4 (&w)[CW][P], f32x16 (&acc)[RW][CW])
    {
        BPlanes<P> A[RW], B[CW];
#pragma unroll
        for (int i = 0; i < RW; ++i) A[i] = b3_split8<P>(x[i][0], x[i][1]);
#pragma unroll
        for (int j = 0; j < CW; ++j)
#pragma unroll
            for (int pl = 0; pl < P; ++pl) B[j].p[pl] = w[j][pl];
        mfma6_all<P, RW, CW>(A, B, acc);
    }
};
using Gemm32Split = Gemm32Planes<3>;

template <int P, int RW, int CW, int SK>
__global__ __launch_bounds__(SK > 4 ? 64 * SK : 256) void gemm32b_kernel(Gemm32Args a)
{
    using Op = Gemm32Planes<P>;
#include "gemm32_frame_body.h"
}

}  // namespace

// [cin, cout] row-major, cin % 16 == 0, cout % 32 == 0  ->  cin * cout * planes uint16 (planes = 3: the exact split, 1: rounded to nearest even):
//   image[(((cb * nq + q) * planes + plane) * 64 + lane) * 8 + t] = piece `plane` of W[16 q + 8 (lane >> 5) + t][32 cb + (lane & 31)]
void pack_p32b(const float* W, int cin, int cout, uint16_t* out, int planes)
{
    const int nq = cin / 16, ncb = cout / 32;
    for (int cb = 0; cb < ncb; ++cb)
        for (int q = 0; q < nq; ++q)
            for (int pl = 0; pl < planes; ++pl)
                for (int lane = 0; lane < 64; ++lane)
                    for (int t = 0; t < 8; ++t) {
                        const int k = 16 * q + 8 * (lane >> 5) + t, n = 32 * cb + (lane & 31);
                        out[((((size_t)cb * nq + q) * planes + pl) * 64 + lane) * 8 + t] = b3_plane_of(W[(size_t)k * cout + n], pl, planes);
                    }
}

bool gemm32b_fits(const PackedLinear& L, const RowSrc& s1, const RowSrc& s2, int64_t R, int ldy)
{
    return gemm32_fits_kc(L.round ? L.w32b1 : L.w32b, Gemm32Split::KC, L, s1, s2, R, ldy);
}

Gemm32Plan gemm32b_plan(const Tuning& tn, int64_t R, int cin, int cout, int planes)
{
    Gemm32Plan p;
    const int rblocks = (int)((R + 31) / 32);
    // two column blocks per wave (an activation split feeds twelve MFMAs) whenever the layer has them; two row blocks per wave (a weight
    // fragment feeds both: half the weight stream) once that still leaves every SIMD a wave
    p.cw = cout % 64 == 0 ? 2 : 1;
    p.rw = (int64_t)(rblocks / 2) * (cout / (32 * p.cw)) >= 1024 ? 2 : 1;
    // (A/B overrides of the tile shape, Tuning::gemm32b_rw / _cw: only the compiled shapes 1 and 2; anything else is ignored)
    if (tn.gemm32b_rw == 1 || tn.gemm32b_rw == 2) p.rw = tn.gemm32b_rw;
    if ((tn.gemm32b_cw == 1 || tn.gemm32b_cw == 2) && cout % (32 * tn.gemm32b_cw) == 0) p.cw = tn.gemm32b_cw;
    p.cgroups = cout / (32 * p.cw);
    const int runits = (rblocks + p.rw - 1) / p.rw;
    // split K across the waves of a workgroup while the plain grid leaves SIMDs idle (1 024 of them) and the slices keep >= 4 chunks
    const int64_t units = (int64_t)runits * p.cgroups;
    p.sk = 1;
    // (eight waves per workgroup -- gemm32.hip's form for the long-K layers -- measured SLOWER here: dec1 24.8 -> 30.8 us, pipelined step
    //  0.857 -> 0.875 ms: twice the partial sums through LDS for a chain that the register ring already keeps fed)
    while (p.sk < 4 && units * p.sk < 1536 && cin / 16 / (p.sk * 2) >= 4) p.sk *= 2;
    const int ru_per_wg = 4 / p.sk;
    p.rgroups = (runits + ru_per_wg - 1) / ru_per_wg;
    p.pd = planes == 1 ? gemm32b1_pd() : gemm32b_pd(p.rw, p.cw);
    return p;
}

int gemm32b(ps_context* c, const PackedLinear& L, const RowSrc& s1, const RowSrc& s2, int64_t R, float* y, int ldy)
{
    if (R <= 0) return PS_OK;
    PS_CHECK(gemm32b_fits(L, s1, s2, R, ldy), "gemm32b: shape / alignment not supported (cin %d, cout %d)", L.cin, L.cout);
    // a layer of rounded operands (PackedLinear::round, PS_PREC_BF16) runs the one-plane kernels on its one-plane image: the same plan
    const int planes = L.round ? 1 : 3;
    const Gemm32Plan p = gemm32b_plan(c->tune, R, L.cin, L.cout, planes);
    const Gemm32Args a = gemm32_args(L.round ? L.w32b1 : L.w32b, L, s1, s2, R, y, ldy, p);
    const int rw = p.rw, cw = p.cw, sk = p.sk;
    const unsigned grid = 8u * (unsigned)((a.rgroups * a.cgroups + 7) / 8);
    const dim3 block(256);
#define PS_G32B_P(P_, RW_, CW_)                                                                                          \
    if (sk == 1) hipLaunchKernelGGL((gemm32b_kernel<P_, RW_, CW_, 1>), dim3(grid), block, 0, c->stream, a);              \
    else if (sk == 2) hipLaunchKernelGGL((gemm32b_kernel<P_, RW_, CW_, 2>), dim3(grid), block, 0, c->stream, a);         \
    else hipLaunchKernelGGL((gemm32b_kernel<P_, RW_, CW_, 4>), dim3(grid), block, 0, c->stream, a)
#define PS_G32B(RW_, CW_)                      \
    if (planes == 1) { PS_G32B_P(1, RW_, CW_); } \
    else { PS_G32B_P(3, RW_, CW_); }
    if (rw == 2 && cw == 2) { PS_G32B(2, 2) }
    else if (rw == 2) { PS_G32B(2, 1) }
    else if (cw == 2) { PS_G32B(1, 2) }
    else { PS_G32B(1, 1) }
#undef PS_G32B_P
#undef PS_G32B
    PS_HIP(hipGetLastError());
    return PS_OK;
}

}  // namespace ps
