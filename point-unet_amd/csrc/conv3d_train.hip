// conv3d_train.hip -- the gradients of conv3d.hip's convolution (include/pointseg_saliency_train.h; the instance norm's
// gradient is saliency_train.hip's), with the forward's guarantees: exact fp32 operands on v_mfma_f32_16x16x4_f32 (mfma_tile.h's fragment
// maps), float64 fixed-order slab sums, no float atomic, two runs give the same bytes.
//
// Data gradient: a gather, the forward's implicit GEMM with the roles turned.  Rows are the voxels i of the virtual (concatenated,
// up-sampled) input, columns its channels, k = tap * C_out + co;  A[i, k] = dy[o, co] with o = (i + pad - t * dilation) / stride where that
// is a whole number inside the output (0 elsewhere; never materialised), B[k, ci] = w[t, ci, co] -- a transposed copy of the kernel in
// scratch, the one thing that is repacked.  With up == 1 the tile is written straight into dx / dx2 (the columns split at C1); with
// up > 1 it goes to scratch and a second kernel adds each source voxel's up^3 virtual voxels in one fixed order.
// Weight gradient: dw[(t, ci), co] = sum over voxels of in[v, (t, ci)] . dy[v, co] -- rows (t, ci) plus ONE more row of ones, whose
// product is the bias gradient; the reduction over the output voxels is cut into slabs of 4096 per sample, a workgroup writes its slab's
// [rows, columns] tile to scratch, and reduce_partials.h adds the slabs in one fixed order in float64.  `in` is fetched as the forward
// fetches it (concat, / up, 0 in the padding).
// Rounding (both): a chunk of 32 k is summed in a fresh accumulator and then added to the running one, as in conv3d.hip.
// The data gradient is the forward's kernel with its compile-time gather policy: conv3d_kernel<RT, NT, GRAD = true> (conv3d_bf16.hip's
// conv3d_b_kernel at the other precisions) differs from the forward in the row's corner, the fetch's coordinate step and the epilogue's
// column split, each behind `if constexpr`, so the forward's instantiations stay what they are.  The entry below describes the op once,
// as a Conv3dArgs with the grad fields (saliency.h), and conv3d_launch picks the pipe.
// At PS_PREC_BF16X3 / PS_PREC_BF16 (include/pointseg_saliency_train_precision.h) the same entries run the bf16 matrix pipe,
// the weight gradient through conv3d_train_bf16.hip; the transposed kernel copy, the up-sampling's sum, the slab partials and their float64
// reduction are the ones below.  conv3d_kit.h holds what the four sources share.
#include "../../include/pointseg_saliency_train_precision.h"
#include "conv3d_kit.h"
#include "reduce_partials.h"
#include "scratch.h"

namespace ps {

namespace {

// ---- data gradient -----------------------------------------------------------------------------------------------------------------------------

// wt[(tap * cout + co) * cin + ci] = w[(tap * cin + ci) * cout + co]
__global__ __launch_bounds__(256) void transpose_kernel_kernel(const float* __restrict__ w, unsigned total, int cin, int cout, float* __restrict__ wt)
{
    const unsigned e = blockIdx.x * 256u + threadIdx.x;
    if (e >= total) return;
    const unsigned ci = e % cin, r = e / cin, co = r % cout, tap = r / cout;
    wt[e] = w[((size_t)tap * cin + ci) * cout + co];
}

// grid (ceil(Vs * ncols / 256), B): a source voxel's gradient = the sum of g over its up^3 virtual voxels, (dz, dy, dx) ascending
__global__ __launch_bounds__(256) void upsample_bwd_kernel(const float* __restrict__ g, int ncols, int c0, int Ds, int Hs, int Ws, int up, int C1, int C2,
                                                           float* __restrict__ dx, float* __restrict__ dx2)
{
    const unsigned e = blockIdx.x * 256u + threadIdx.x;
    const unsigned Vs = (unsigned)(Ds * Hs * Ws);
    if (e >= Vs * (unsigned)ncols) return;
    const unsigned c = e % ncols, s = e / ncols;
    const int sx = s % Ws, sy = s / Ws % Hs, sz = s / (Ws * Hs);
    const int H = Hs * up, W = Ws * up;
    const float* gb = g + (size_t)blockIdx.y * Vs * up * up * up * ncols + c;
    float sum = 0.f;
    for (int dz = 0; dz < up; ++dz)
        for (int dy = 0; dy < up; ++dy)
            for (int dxx = 0; dxx < up; ++dxx)
                sum += gb[(size_t)(((sz * up + dz) * H + sy * up + dy) * W + sx * up + dxx) * ncols];
    const int col = c0 + (int)c;
    const size_t row = (size_t)blockIdx.y * Vs + s;
    if (col < C1) dx[row * C1 + col] = sum;
    else dx2[row * C2 + (col - C1)] = sum;
}

// ---- weight and bias gradient ------------------------------------------------------------------------------------------------------------------

// grid (mtiles * B * slabs, column tiles).  Both tiles are k-major in LDS (k = a voxel of the slab): thread t fetches rows t % 64 (+ 64)
// -- adjacent lanes adjacent input channels -- of the voxels t / 64 + 4 i, whose input corners come from LDS.
template <int RT, int NT>
__global__ __launch_bounds__(256) void conv3d_bwd_weight_kernel(BwdWeightArgs a)
{
    constexpr int M = 64 * RT, N = 16 * NT;
    constexpr int PA = M + 16;  // 16 (mod 32) floats
    constexpr int BI = kKC * N / 256;
    constexpr int BKS = 256 / N;
    __shared__ float As[kKC * PA];
    __shared__ float Bs[kKC * kBP];
    __shared__ int4 vox[2][kKC];  // the input corner of the voxel's receptive field (z, y, x) and whether the voxel exists

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int mt = blockIdx.x % a.mtiles, pidx = blockIdx.x / a.mtiles;
    const int b = pidx / a.slabs, slab = pidx - b * a.slabs;
    const int m0 = mt * M, n0 = blockIdx.y * N;
    const int Vo = a.Do * a.Ho * a.Wo;
    const int v0 = slab * kWSlab, v1 = min(Vo, v0 + kWSlab);
    const int nchunks = (v1 - v0 + kKC - 1) / kKC;
    const int cin = a.C1 + a.C2;
    const size_t xs = (size_t)a.Ds * a.Hs * a.Ws;
    const float* dyb = a.dy + (size_t)b * Vo * a.cout;

    // this thread's rows: kind 0 = none, 1 = a kernel row, 2 = the row of ones
    int kind[RT], rdz[RT], rdy[RT], rdx[RT], rld[RT];
    const float* rsrc[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        const int lr = m0 + rt * 64 + lane, row = a.r0 + lr;
        kind[rt] = lr >= a.nrows ? 0 : (row < a.Ktot ? 1 : 2);
        const int tap = kind[rt] == 1 ? row / cin : 0, ci = kind[rt] == 1 ? row - tap * cin : 0;
        rdx[rt] = (tap % a.kw) * a.dil, rdy[rt] = (tap / a.kw % a.kh) * a.dil, rdz[rt] = (tap / (a.kw * a.kh)) * a.dil;
        const bool second = ci >= a.C1;
        rsrc[rt] = second ? a.x2 + (size_t)b * xs * a.C2 + (ci - a.C1) : a.x + (size_t)b * xs * a.C1 + ci;
        rld[rt] = second ? a.C2 : a.C1;
    }
    const int bcol = t % N, bk = t / N;

    auto put_vox = [&](int chunk) {
        if (t < kKC) {
            const int v = v0 + chunk * kKC + t;
            int4 vi = {0, 0, 0, 0};
            if (v < v1) vi = {v / (a.Wo * a.Ho) * a.stride - a.pd, v / a.Wo % a.Ho * a.stride - a.ph, v % a.Wo * a.stride - a.pw, 1};
            vox[chunk & 1][t] = vi;
        }
    };

    float areg[RT][8], breg[BI];
    auto fetch = [&](int chunk) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int4 vi = vox[chunk & 1][wave + 4 * i];
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                int z = vi.x + rdz[rt], y = vi.y + rdy[rt], x = vi.z + rdx[rt];
                const bool ok = kind[rt] == 1 && vi.w && (unsigned)z < (unsigned)a.D && (unsigned)y < (unsigned)a.H && (unsigned)x < (unsigned)a.W;
                if (!ok) z = y = x = 0;
                if (a.up > 1) {
                    z = (int)((unsigned)z / (unsigned)a.up);
                    y = (int)((unsigned)y / (unsigned)a.up);
                    x = (int)((unsigned)x / (unsigned)a.up);
                }
                const float one = (kind[rt] == 2 && vi.w) ? 1.f : 0.f;
                areg[rt][i] = ok ? rsrc[rt][(size_t)((z * a.Hs + y) * a.Ws + x) * rld[rt]] : one;
            }
        }
#pragma unroll
        for (int i = 0; i < BI; ++i) {
            const int v = v0 + chunk * kKC + bk + BKS * i;
            breg[i] = (v < v1 && n0 + bcol < a.cout) ? dyb[(size_t)v * a.cout + n0 + bcol] : 0.f;
        }
    };

    f32x4 acc[RT][NT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[rt][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    put_vox(0);
    __syncthreads();
    fetch(0);
    // A[i][k]: lane = i + 16 * k, B[k][j]: lane = j + 16 * k -- both read row (lane / 16) of the k-step, column lane % 16 of their tile
    const float* a0 = As + (lane >> 4) * PA + wave * RT * 16 + (lane & 15);
    const float* b0 = Bs + (lane >> 4) * kBP + (lane & 15);
#pragma unroll 1
    for (int chunk = 0; chunk < nchunks; ++chunk) {
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) As[(wave + 4 * i) * PA + rt * 64 + lane] = areg[rt][i];
#pragma unroll
        for (int i = 0; i < BI; ++i) Bs[(bk + BKS * i) * kBP + bcol] = breg[i];
        if (chunk + 1 < nchunks) put_vox(chunk + 1);
        __syncthreads();
        if (chunk + 1 < nchunks) fetch(chunk + 1);
        chunk_mma<RT, NT>(a0, 16, 4 * PA, b0, acc);
        __syncthreads();
    }

    float* pb = a.part + (size_t)pidx * a.nrows * a.cout;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int col = n0 + j * 16 + (lane & 15);
        if (col >= a.cout) continue;
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int lr = m0 + wave * RT * 16 + rt * 16 + (lane >> 4) * 4 + r;
                if (lr < a.nrows) pb[(size_t)lr * a.cout + col] = acc[rt][j][r];
            }
    }
}

template <int RT, int NT>
void launch_weight(hipStream_t sm, BwdWeightArgs& a)
{
    a.mtiles = ceil_div(a.nrows, 64 * RT);
    const dim3 grid((unsigned)((int64_t)a.mtiles * a.B * a.slabs), (unsigned)ceil_div(a.cout, 16 * NT));
    hipLaunchKernelGGL((conv3d_bwd_weight_kernel<RT, NT>), grid, dim3(256), 0, sm, a);
}

}  // namespace

}  // namespace ps

extern "C" int ps_conv3d_bwd_data(ps_context* c, const void* dy, const void* w, int64_t B, int64_t Ds, int64_t Hs, int64_t Ws, int64_t C1, int64_t C2, int32_t up,
                                  int32_t kd, int32_t kh, int32_t kw, int64_t C_out, int32_t stride, int32_t dilation, void* dx, void* dx2, void* scratch,
                                  int64_t* scratch_bytes)
{
    return ps_conv3d_bwd_data_prec(c, dy, w, B, Ds, Hs, Ws, C1, C2, up, kd, kh, kw, C_out, stride, dilation, dx, dx2, scratch, scratch_bytes, PS_PREC_FP32);
}

extern "C" int ps_conv3d_bwd_data_prec(ps_context* c, const void* dy, const void* w, int64_t B, int64_t Ds, int64_t Hs, int64_t Ws, int64_t C1, int64_t C2,
                                       int32_t up, int32_t kd, int32_t kh, int32_t kw, int64_t C_out, int32_t stride, int32_t dilation, void* dx, void* dx2,
                                       void* scratch, int64_t* scratch_bytes, int32_t precision)
{
    using namespace ps;
    const char* who = precision == PS_PREC_FP32 ? "ps_conv3d_bwd_data" : "ps_conv3d_bwd_data_prec";
    PS_TRY(precision_check(who, precision));
    PS_CHECK(scratch_bytes, "%s: NULL scratch_bytes", who);
    PS_TRY(conv_geometry_ok(who, B, Ds, Hs, Ws, C1, C2, up, kd, kh, kw, C_out, stride, dilation));
    const int cin = (int)(C1 + C2), taps = kd * kh * kw;
    const int D = (int)Ds * up, H = (int)Hs * up, W = (int)Ws * up;
    Carver cv{static_cast<char*>(scratch)};
    float* wt = cv.take<float>((size_t)taps * cin * C_out);
    float* g = up > 1 ? cv.take<float>((size_t)B * D * H * W * cin) : nullptr;
    if (!scratch) {
        *scratch_bytes = (int64_t)cv.off;
        return PS_OK;
    }
    PS_CHECK(dy && w, "%s: NULL dy or w (they may be NULL only in the call that sizes the scratch)", who);
    PS_CHECK(C2 > 0 || !dx2, "%s: dx2 must be NULL when C2 == 0", who);
    PS_CHECK(dx || dx2, "%s: every result is NULL", who);
    PS_CHECK(dx != dy && dx2 != dy, "%s: dx and dx2 must not overlap dy", who);
    PS_CHECK(c, "%s: NULL context", who);
    PS_TRY(check_scratch(who, scratch, scratch_bytes, cv.off));

    // the forward's kernels on the turned roles (saliency.h's grad fields): their "input" is dy, their rows the virtual input's voxels, their
    // columns the channels [c0, c0 + ncols) of the virtual input that this call computes
    const int c0 = dx ? 0 : (int)C1, ncols = (dx2 ? cin : (int)C1) - c0;
    Conv3dArgs a = {};
    a.x = static_cast<const float*>(dy), a.w = wt + c0, a.ldw = cin, a.grad = 1, a.precision = precision;
    a.B = (int)B, a.C1 = a.ldx = (int)C_out, a.up = 1, a.cout = ncols;
    a.Do = D, a.Ho = H, a.Wo = W;
    a.Ds = a.D = same_out(D, stride), a.Hs = a.H = same_out(H, stride), a.Ws = a.W = same_out(W, stride);
    a.kd = kd, a.kh = kh, a.kw = kw, a.stride = stride, a.dil = dilation;
    a.pd = same_pad_before(D, kd, stride, dilation), a.ph = same_pad_before(H, kh, stride, dilation), a.pw = same_pad_before(W, kw, stride, dilation);
    // up == 1: straight into dx / dx2, the columns split at C1; else the whole tile to scratch, for upsample_bwd_kernel
    if (up > 1) a.y = g, a.ldy = ncols, a.nsplit = cin - c0;
    else a.y = static_cast<float*>(dx), a.ldy = (int)C1, a.y2 = static_cast<float*>(dx2), a.ldy2 = (int)C2, a.nsplit = (int)C1 - c0;
    // PS_PREC_BF16X3 keeps the fp32 kernel where dy does not take the 16-byte fetch (conv3d_bwd_weight_split_pays' comment)
    if (precision == PS_PREC_BF16X3 && !conv3d_b_vec(a)) a.precision = PS_PREC_FP32;

    PS_HIP(hipSetDevice(c->device));
    hipStream_t sm = c->stream;
    Stage stg(c, "conv3d_bwd_data", 3);
    const unsigned wn = (unsigned)((size_t)taps * cin * C_out);
    hipLaunchKernelGGL(transpose_kernel_kernel, dim3(blocks256(wn)), dim3(256), 0, sm, static_cast<const float*>(w), wn, cin, (int)C_out, wt);
    conv3d_launch(sm, a);
    if (up > 1)
        hipLaunchKernelGGL(upsample_bwd_kernel, dim3(blocks256((size_t)Ds * Hs * Ws * ncols), (unsigned)B), dim3(256), 0, sm, g, ncols, c0, (int)Ds, (int)Hs,
                           (int)Ws, (int)up, (int)C1, (int)C2, static_cast<float*>(dx), static_cast<float*>(dx2));
    PS_HIP(hipGetLastError());
    return PS_OK;
}

extern "C" int ps_conv3d_bwd_weight(ps_context* c, const void* x, const void* x2, const void* dy, int64_t B, int64_t Ds, int64_t Hs, int64_t Ws, int64_t C1,
                                    int64_t C2, int32_t up, int32_t kd, int32_t kh, int32_t kw, int64_t C_out, int32_t stride, int32_t dilation, void* dw,
                                    void* dbias, void* scratch, int64_t* scratch_bytes)
{
    return ps_conv3d_bwd_weight_prec(c, x, x2, dy, B, Ds, Hs, Ws, C1, C2, up, kd, kh, kw, C_out, stride, dilation, dw, dbias, scratch, scratch_bytes,
                                     PS_PREC_FP32);
}

extern "C" int ps_conv3d_bwd_weight_prec(ps_context* c, const void* x, const void* x2, const void* dy, int64_t B, int64_t Ds, int64_t Hs, int64_t Ws,
                                         int64_t C1, int64_t C2, int32_t up, int32_t kd, int32_t kh, int32_t kw, int64_t C_out, int32_t stride,
                                         int32_t dilation, void* dw, void* dbias, void* scratch, int64_t* scratch_bytes, int32_t precision)
{
    using namespace ps;
    const char* who = precision == PS_PREC_FP32 ? "ps_conv3d_bwd_weight" : "ps_conv3d_bwd_weight_prec";
    PS_TRY(precision_check(who, precision));
    PS_CHECK(scratch_bytes, "%s: NULL scratch_bytes", who);
    PS_TRY(conv_geometry_ok(who, B, Ds, Hs, Ws, C1, C2, up, kd, kh, kw, C_out, stride, dilation));
    Conv3dArgs f = {};
    f.B = (int)B, f.Ds = (int)Ds, f.Hs = (int)Hs, f.Ws = (int)Ws, f.C1 = (int)C1, f.C2 = (int)C2, f.up = up;
    f.kd = kd, f.kh = kh, f.kw = kw, f.cout = (int)C_out, f.stride = stride, f.dil = dilation;
    conv3d_plan(f);
    const int Ktot = kd * kh * kw * (int)(C1 + C2);
    const int slabs = ceil_div((int64_t)f.Do * f.Ho * f.Wo, kWSlab);
    const int64_t n_part = B * slabs;
    PS_CHECK(n_part * ceil_div(Ktot + 1, 64) < (1ll << 31), "%s: B = %lld times %d slabs of %d output voxels are more workgroups than one launch holds", who,
             (long long)B, slabs, kWSlab);
    Carver cv{static_cast<char*>(scratch)};
    float* part = cv.take<float>((size_t)n_part * (Ktot + 1) * C_out);
    if (!scratch) {
        *scratch_bytes = (int64_t)cv.off;
        return PS_OK;
    }
    PS_CHECK(x && dy, "%s: NULL x or dy (they may be NULL only in the call that sizes the scratch)", who);
    PS_CHECK((C2 == 0) == (x2 == nullptr), "%s: x2 must be given exactly when C2 > 0", who);
    PS_CHECK(dw || dbias, "%s: every result is NULL", who);
    PS_CHECK(c, "%s: NULL context", who);
    PS_TRY(check_scratch(who, scratch, scratch_bytes, cv.off));

    BwdWeightArgs a = {};
    a.x = static_cast<const float*>(x), a.x2 = static_cast<const float*>(x2), a.dy = static_cast<const float*>(dy), a.part = part;
    a.r0 = dw ? 0 : Ktot;
    a.nrows = (dbias ? Ktot + 1 : Ktot) - a.r0;
    a.Ktot = Ktot, a.slabs = slabs;
    a.B = f.B, a.Ds = f.Ds, a.Hs = f.Hs, a.Ws = f.Ws, a.C1 = f.C1, a.C2 = f.C2, a.up = up, a.D = f.D, a.H = f.H, a.W = f.W, a.Do = f.Do, a.Ho = f.Ho, a.Wo = f.Wo;
    a.cout = f.cout, a.kd = kd, a.kh = kh, a.kw = kw, a.stride = stride, a.dil = dilation, a.pd = f.pd, a.ph = f.ph, a.pw = f.pw;

    PS_HIP(hipSetDevice(c->device));
    hipStream_t sm = c->stream;
    Stage stg(c, "conv3d_bwd_weight", 2);
    if (precision == PS_PREC_BF16 || (precision == PS_PREC_BF16X3 && conv3d_bwd_weight_split_pays(a.C1 + a.C2, a.cout)))
        conv3d_bwd_weight_b_launch(sm, a, precision);
    else conv_form(a.nrows > 64, a.cout, [&](auto rt, auto nt) { launch_weight<decltype(rt)::value, decltype(nt)::value>(sm, a); });
    const int nv = a.nrows * a.cout, n0 = dw ? Ktot * a.cout : 0;
    hipLaunchKernelGGL((reduce_partials2_kernel<float, double>), dim3((unsigned)ceil_div(nv, 16)), dim3(256), 0, sm, part, (int)n_part, nv, n0,
                       static_cast<float*>(dw), static_cast<float*>(dbias));
    PS_HIP(hipGetLastError());
    return PS_OK;
}
