// conv3d.hip -- one implicit-GEMM 3-D convolution, channels last, on v_mfma_f32_16x16x4_f32 (exact fp32; mfma_tile.h's fragment maps):
// ps_conv3d and the layers of ps_saliency_forward (include/pointseg_saliency.h).
//
// The product is  Y[v, co] = sum over k of A[v, k] . Wm[k, co]  with v an output voxel of one sample, k = tap * C_in + ci -- TensorFlow's
// kernel layout [kd, kh, kw, C_in, C_out] IS the row-major [K, C_out] matrix, so no weight is repacked -- and A[v, k] the input voxel that
// tap reaches, 0 where the tap falls into the SAME padding.  A is never materialised: a workgroup of four waves owns 64 * RT output voxels
// and 16 * NT output channels, walks K in chunks of 32, and per chunk every thread fetches its A elements (one k column, 8 * RT rows:
// the tap and the channel are decoded once per chunk, the row's input corner comes from LDS) and its Wm elements into registers, stores them
// to LDS, and the fetch of the next chunk is in flight while the waves run the chunk's 8 k-steps of MFMA.  The channel concat of two
// sources and the nearest up-sampling are part of that fetch (channel >= C1 reads x2; coordinate / up).
// Rounding: a chunk is summed in a fresh accumulator and then added to the running one, so the dependent chain of a K = 10 368 layer is
// 32 + 324 roundings long (an MFMA is an ordered chain of its four products) and not 10 368.
#include "conv3d_kit.h"

namespace ps {

namespace {

// GRAD: the data gradient (saliency.h's grad fields) -- the same implicit GEMM with the roles turned.  The row's corner
// (conv3d_kit.h's conv_row), the fetch's coordinate step and the epilogue's column split are the whole difference, each behind
// `if constexpr`, so the forward compiles to what it was.
template <int RT, int NT, bool GRAD>
__global__ __launch_bounds__(256) void conv3d_kernel(Conv3dArgs a)
{
    constexpr int M = 64 * RT, N = 16 * NT;
    constexpr int AI = M / 8;            // A elements per thread and chunk
    constexpr int BI = kKC * N / 256;    // B elements per thread and chunk
    constexpr int BKS = 256 / N;         // k rows between a thread's B elements
    __shared__ float As[M * kAP];
    __shared__ float Bs[kKC * kBP];
    __shared__ int4 rows[M];  // conv_row: the input corner of the row's receptive field (GRAD: the row's voxel + pad) and whether the row exists

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int b = blockIdx.z, n0 = blockIdx.y * N, m0 = blockIdx.x * M;
    const int Vo = a.Do * a.Ho * a.Wo;
    for (int r = t; r < M; r += 256) rows[r] = conv_row<GRAD>(a, m0 + r, Vo);
    __syncthreads();

    const int cin = a.C1 + a.C2;
    const int Ktot = a.kd * a.kh * a.kw * cin;
    const int nchunks = (Ktot + kKC - 1) / kKC;
    const int akk = t & 31, arow = t >> 5;
    const int bcol = t % N, bk = t / N;
    const size_t xs = (size_t)a.Ds * a.Hs * a.Ws;  // voxels of one source sample
    const float* xb = a.x + (size_t)b * xs * a.ldx;
    const float* x2b = a.x2 ? a.x2 + (size_t)b * xs * a.ldx2 : nullptr;
    const float* wb = a.w + (size_t)b * a.w_bstride;
    const bool s2 = a.stride == 2;  // (GRAD)

    float areg[AI], breg[BI];
    auto fetch = [&](int chunk) {
        const int k = chunk * kKC + akk;
        const bool kin = k < Ktot;
        const int tap = kin ? k / cin : 0, ci = kin ? k - tap * cin : 0;
        const int dx = (tap % a.kw) * a.dil, dy = (tap / a.kw % a.kh) * a.dil, dz = (tap / (a.kw * a.kh)) * a.dil;
        const bool second = !GRAD && ci >= a.C1;  // (the gradient's operand is dy alone, not up-sampled)
        const float* src = second ? x2b + (ci - a.C1) : xb + ci;
        const int ld = second ? a.ldx2 : a.ldx;
#pragma unroll
        for (int i = 0; i < AI; ++i) {
            const int4 ri = rows[arow + 8 * i];
            int z, y, x;
            bool ok;
            if constexpr (GRAD) {
                z = ri.x - dz, y = ri.y - dy, x = ri.z - dx;  // o * stride
                ok = kin && ri.w && (z | y | x) >= 0;
                if (s2) {
                    ok = ok && ((z | y | x) & 1) == 0;
                    z >>= 1, y >>= 1, x >>= 1;
                }
                ok = ok && z < a.D && y < a.H && x < a.W;
            } else {
                z = ri.x + dz, y = ri.y + dy, x = ri.z + dx;
                ok = kin && ri.w && (unsigned)z < (unsigned)a.D && (unsigned)y < (unsigned)a.H && (unsigned)x < (unsigned)a.W;
            }
            if (!ok) z = y = x = 0;
            if (!GRAD && a.up > 1) {
                z = (int)((unsigned)z / (unsigned)a.up);
                y = (int)((unsigned)y / (unsigned)a.up);
                x = (int)((unsigned)x / (unsigned)a.up);
            }
            areg[i] = ok ? src[(size_t)((z * (GRAD ? a.H : a.Hs) + y) * (GRAD ? a.W : a.Ws) + x) * ld] : 0.f;  // (GRAD: the operand is not up-sampled)
        }
#pragma unroll
        for (int i = 0; i < BI; ++i) {
            const int kb = chunk * kKC + bk + BKS * i;
            breg[i] = (kb < Ktot && n0 + bcol < a.cout) ? wb[(size_t)kb * (GRAD ? a.ldw : a.cout) + n0 + bcol] : 0.f;
        }
    };

    f32x4 acc[RT][NT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[rt][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    fetch(0);
    const float* a0 = As + (wave * RT * 16 + (lane & 15)) * kAP + (lane >> 4);
    const float* b0 = Bs + (lane >> 4) * kBP + (lane & 15);
#pragma unroll 1
    for (int chunk = 0; chunk < nchunks; ++chunk) {
#pragma unroll
        for (int i = 0; i < AI; ++i) As[(arow + 8 * i) * kAP + akk] = areg[i];
#pragma unroll
        for (int i = 0; i < BI; ++i) Bs[(bk + BKS * i) * kBP + bcol] = breg[i];
        __syncthreads();
        if (chunk + 1 < nchunks) fetch(chunk + 1);
        chunk_mma<RT, NT>(a0, 16 * kAP, 4, b0, acc);
        __syncthreads();
    }

    // C[i][j]: lane = j + 16 * (i / 4), reg = i % 4
    float* yb = a.y + (size_t)b * Vo * a.ldy;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int col = n0 + j * 16 + (lane & 15);
        if (col >= a.cout) continue;
        if constexpr (GRAD) {
            const bool first = col < a.nsplit;
            float* o = first ? yb + col : a.y2 + (size_t)b * Vo * a.ldy2 + (col - a.nsplit);
            const int ld = first ? a.ldy : a.ldy2;
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int v = m0 + wave * RT * 16 + rt * 16 + (lane >> 4) * 4 + r;
                    if (v < Vo) o[(size_t)v * ld] = acc[rt][j][r];
                }
        } else {
            const float bias = a.bias ? a.bias[col] : 0.f;
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int v = m0 + wave * RT * 16 + rt * 16 + (lane >> 4) * 4 + r;
                    if (v < Vo) yb[(size_t)v * a.ldy + col] = acc[rt][j][r] + bias;
                }
        }
    }
}

template <int RT, int NT>
void launch(hipStream_t sm, const Conv3dArgs& a)
{
    const int Vo = a.Do * a.Ho * a.Wo;
    const dim3 grid((unsigned)ceil_div(Vo, 64 * RT), (unsigned)ceil_div(a.cout, 16 * NT), (unsigned)a.B);
    if (a.grad) hipLaunchKernelGGL((conv3d_kernel<RT, NT, true>), grid, dim3(256), 0, sm, a);
    else hipLaunchKernelGGL((conv3d_kernel<RT, NT, false>), grid, dim3(256), 0, sm, a);
}

}  // namespace

void conv3d_plan(Conv3dArgs& a)
{
    a.D = a.Ds * a.up;
    a.H = a.Hs * a.up;
    a.W = a.Ws * a.up;
    a.Do = same_out(a.D, a.stride);
    a.Ho = same_out(a.H, a.stride);
    a.Wo = same_out(a.W, a.stride);
    a.pd = same_pad_before(a.D, a.kd, a.stride, a.dil);
    a.ph = same_pad_before(a.H, a.kh, a.stride, a.dil);
    a.pw = same_pad_before(a.W, a.kw, a.stride, a.dil);
}

// (conv3d_kit.h's form rule; the data gradient's rows are the virtual input's voxels and its columns the computed channels)
void conv3d_launch(hipStream_t sm, const Conv3dArgs& a)
{
    if (a.precision != PS_PREC_FP32) return conv3d_b_launch(sm, a);
    conv_form((int64_t)a.Do * a.Ho * a.Wo >= 2048, a.cout, [&](auto rt, auto nt) { launch<decltype(rt)::value, decltype(nt)::value>(sm, a); });
}

}  // namespace ps

extern "C" int ps_conv3d(ps_context* c, const void* x, const void* x2, int64_t B, int64_t Ds, int64_t Hs, int64_t Ws, int64_t C1, int64_t C2, int32_t up,
                         const void* w, const void* bias, int32_t kd, int32_t kh, int32_t kw, int64_t C_out, int32_t stride, int32_t dilation, void* y)
{
    return ps_conv3d_prec(c, x, x2, B, Ds, Hs, Ws, C1, C2, up, w, bias, kd, kh, kw, C_out, stride, dilation, y, PS_PREC_FP32);
}

extern "C" int ps_conv3d_prec(ps_context* c, const void* x, const void* x2, int64_t B, int64_t Ds, int64_t Hs, int64_t Ws, int64_t C1, int64_t C2,
                              int32_t up, const void* w, const void* bias, int32_t kd, int32_t kh, int32_t kw, int64_t C_out, int32_t stride,
                              int32_t dilation, void* y, int32_t precision)
{
    using namespace ps;
    const char* who = precision == PS_PREC_FP32 ? "ps_conv3d" : "ps_conv3d_prec";
    PS_TRY(precision_check(who, precision));
    PS_TRY(conv_geometry_ok(who, B, Ds, Hs, Ws, C1, C2, up, kd, kh, kw, C_out, stride, dilation));
    PS_CHECK(c && x && w && y, "%s: NULL argument", who);
    PS_CHECK((C2 == 0) == (x2 == nullptr), "%s: x2 must be given exactly when C2 > 0", who);
    PS_CHECK(y != x && y != x2, "%s: y must not overlap x or x2", who);

    Conv3dArgs a = {};
    a.x = static_cast<const float*>(x);
    a.x2 = static_cast<const float*>(x2);
    a.w = static_cast<const float*>(w);
    a.bias = static_cast<const float*>(bias);
    a.y = static_cast<float*>(y);
    a.B = (int)B, a.Ds = (int)Ds, a.Hs = (int)Hs, a.Ws = (int)Ws, a.C1 = (int)C1, a.C2 = (int)C2, a.ldx = (int)C1, a.ldx2 = (int)C2, a.up = up;
    a.kd = kd, a.kh = kh, a.kw = kw, a.cout = (int)C_out, a.stride = stride, a.dil = dilation, a.ldy = (int)C_out;
    a.w_bstride = 0;
    a.precision = precision;
    conv3d_plan(a);
    PS_HIP(hipSetDevice(c->device));
    Stage stg(c, "conv3d", 1);
    conv3d_launch(c->stream, a);
    PS_HIP(hipGetLastError());
    return PS_OK;
}
