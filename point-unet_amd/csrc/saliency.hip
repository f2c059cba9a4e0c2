// saliency.hip -- the saliency attention network around conv3d.hip (include/pointseg_saliency.h): instance norm + ReLU,
// the channel and the spatial attention, softmax, the graph of unet3d_attention behind one call, and the window average.  The graph's
// convolutions run at the precision of include/pointseg_saliency_precision.h (conv3d_launch switches); nothing else here depends on it.
//
// Instance norm: per (sample, channel) sum and sum of squares in float64 by saliency_kit.h's slab-sum frame -- a workgroup adds a slab of
// 4096 voxels, its threads in a fixed order, reduce_partials.h adds the slabs in a fixed order -- so two runs give the same bytes and
// E[x^2] - E[x]^2 keeps 53 bits under a mean that dwarfs the deviation.  The apply pass is in place and carries the residual add of a
// Unet3dBlock.  The channel attention's dense part, the spatial gate and the softmax are the kit's too: saliency_train.hip's ops run the same code.
// Concats are never copied: a convolution writes its channels into the concat's buffer (channel pitch ldy), the norm and the next
// convolution read them there (ldx).  The channel attention's per-sample scale goes into C345_conv's kernel, not over the 384-channel tensor.
#include <algorithm>

#include "saliency.h"
#include "saliency_kit.h"
#include "saliency_net.h"

namespace ps {

namespace {

// ---- instance norm + ReLU ----------------------------------------------------------------------------------------------------------------------

// tot[(b * C + c) * 2 + {0, 1}] -> coef[b * C + c] = (mean, gamma / sqrt(var + eps))
__global__ __launch_bounds__(256) void in_coef_kernel(const double* __restrict__ tot, int V, int C, int BC, const float* __restrict__ gamma, float eps,
                                                      float2* __restrict__ coef)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= BC) return;
    const double2 m = moments(tot, i, V, eps);
    coef[i] = make_float2((float)m.x, (float)((double)gamma[i % C] / m.y));
}

// grid (ceil(V * C / 256), B): y = max(0, (x - mean) * scale + beta) [+ res]
__global__ __launch_bounds__(256) void in_apply_kernel(const float* __restrict__ x, int ldx, float* __restrict__ y, int ldy, const float* __restrict__ res,
                                                       int ldres, int V, int C, const float2* __restrict__ coef, const float* __restrict__ beta)
{
    const unsigned e = blockIdx.x * 256u + threadIdx.x;
    if (e >= (unsigned)V * (unsigned)C) return;
    const unsigned v = e / (unsigned)C, c = e - v * (unsigned)C;
    const size_t row = (size_t)blockIdx.y * V + v;
    const float2 cf = coef[blockIdx.y * C + c];
    float o = fmaxf((x[row * ldx + c] - cf.x) * cf.y + beta[c], 0.f);
    if (res) o += res[row * ldres + c];
    y[row * ldy + c] = o;
}

struct NormWs {
    double* part;  // [slabs][B][C][2]
    double* tot;   // [B][C][2]
    float2* coef;  // [B][C]
};

void norm_run(hipStream_t sm, const float* x, int ldx, float* y, int ldy, const float* res, int ldres, int B, int V, int C, const float* gamma,
              const float* beta, float eps, const NormWs& ws)
{
    stats_run(sm, x, ldx, B, V, C, ws.part, ws.tot);
    hipLaunchKernelGGL(in_coef_kernel, dim3(blocks256((size_t)B * C)), dim3(256), 0, sm, ws.tot, V, C, B * C, gamma, eps, ws.coef);
    hipLaunchKernelGGL(in_apply_kernel, dim3(blocks256((size_t)V * C), (unsigned)B), dim3(256), 0, sm, x, ldx, y, ldy, res, ldres, V, C, ws.coef, beta);
}

size_t norm_part_count(int B, int V, int C) { return (size_t)ceil_div(V, kSlab) * B * C * 2; }

// ---- the small ops -------------------------------------------------------------------------------------------------------------------------------

// ChannelWiseAttention3D (attention.py:166-174), one workgroup per sample: the kit's dense part on the statistics pass's sums; the scale
// lands in this sample's copy of C345_conv's [384, 64] kernel.
__global__ __launch_bounds__(256) void ca_fold_kernel(const double* __restrict__ tot, int V, const float* __restrict__ w1, const float* __restrict__ b1,
                                                      const float* __restrict__ w2, const float* __restrict__ b2, const float* __restrict__ wc,
                                                      float* __restrict__ wfold)
{
    __shared__ float mean[kCA], h[kCAh], s[kCA];
    const int t = threadIdx.x, b = blockIdx.x;
    ca_dense(tot + (size_t)b * kCA * 2, 2, V, kCA, kCAh, w1, b1, w2, b2, mean, h, s);
    for (int e = t; e < kCA * kC345; e += 256) wfold[(size_t)b * kCA * kC345 + e] = s[e / kC345] * wc[e];
}

// one thread per voxel: probs = softmax(logits)
template <int MODE>
__global__ __launch_bounds__(256) void softmax_kernel(const float* __restrict__ logits, size_t rows, int C, float* __restrict__ probs)
{
    const size_t r = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    Row<MODE> v;
    row_load<MODE>(logits + r * C, C, v);
    row_softmax<MODE>(C, v);
    row_store<MODE>(probs + r * C, C, v);
}

// dst[r, 0:C] (dense) = src[r, 0:C] (pitch ld): the taps
__global__ __launch_bounds__(256) void copy_rows_kernel(const float* __restrict__ src, int ld, size_t rows, int C, float* __restrict__ dst)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= rows * C) return;
    const size_t r = e / C;
    dst[e] = src[r * ld + (e - r * C)];
}

__global__ __launch_bounds__(256) void window_add_kernel(const float* __restrict__ probs, int p1, int p2, int C, int n0, int n1, int n2, int o0, int o1, int o2,
                                                         int H, int W, float* __restrict__ sum, int* __restrict__ count)
{
    const unsigned e = blockIdx.x * 256u + threadIdx.x;
    if (e >= (unsigned)n0 * n1 * n2 * C) return;
    const unsigned c = e % C, vox = e / C;
    const unsigned k = vox % n2, j = vox / n2 % n1, i = vox / (n2 * n1);
    const size_t dst = ((size_t)(o0 + i) * H + (o1 + j)) * W + (o2 + k);
    sum[dst * C + c] += probs[(((size_t)i * p1 + j) * p2 + k) * C + c];
    if (c == 0) count[dst] += 1;
}

__global__ __launch_bounds__(256) void window_div_kernel(const float* __restrict__ sum, const int* __restrict__ count, unsigned total, int C,
                                                         float* __restrict__ out)
{
    const unsigned e = blockIdx.x * 256u + threadIdx.x;
    if (e >= total) return;
    const int n = count[e / C];
    out[e] = n > 0 ? sum[e] / (float)n : 0.f;
}

// ---- the graph -----------------------------------------------------------------------------------------------------------------------------------

// (the layer table, in the order of include/pointseg_saliency.h, is saliency_net.h's)

}  // namespace

}  // namespace ps

extern "C" int ps_instance_norm_relu(ps_context* c, const void* x, int64_t B, int64_t V, int64_t C, const void* gamma, const void* beta, float eps, void* y,
                                     void* scratch, int64_t* scratch_bytes)
{
    using namespace ps;
    static const char* who = "ps_instance_norm_relu";
    PS_CHECK(scratch_bytes && (c || !scratch), "%s: NULL argument", who);
    PS_TRY(rows_shape_ok(who, B, V, C, 1, 1024, kLimitVC));
    PS_CHECK(eps > 0.f, "%s: eps = %g, must be > 0", who, (double)eps);
    Carver cv{static_cast<char*>(scratch)};
    NormWs ws;
    ws.part = cv.take<double>(norm_part_count((int)B, (int)V, (int)C));
    ws.tot = cv.take<double>((size_t)B * C * 2);
    ws.coef = cv.take<float2>((size_t)B * C);
    if (!scratch) {
        *scratch_bytes = (int64_t)cv.off;
        return PS_OK;
    }
    PS_CHECK(x && y && gamma && beta, "%s: NULL x, y, gamma or beta (they may be NULL only in the call that sizes the scratch)", who);
    PS_TRY(check_scratch(who, scratch, scratch_bytes, cv.off));
    PS_HIP(hipSetDevice(c->device));
    Stage stg(c, "instance_norm_relu", 4);
    norm_run(c->stream, static_cast<const float*>(x), (int)C, static_cast<float*>(y), (int)C, nullptr, 0, (int)B, (int)V, (int)C,
             static_cast<const float*>(gamma), static_cast<const float*>(beta), eps, ws);
    PS_HIP(hipGetLastError());
    return PS_OK;
}

extern "C" int64_t ps_saliency_weight_count(int64_t C_in, int64_t num_classes)
{
    using namespace ps;
    if (!net_args_ok(C_in, num_classes)) {
        set_error("ps_saliency_weight_count: C_in = %lld, num_classes = %lld (1 <= C_in <= 16, 2 <= num_classes <= 16)", (long long)C_in, (long long)num_classes);
        return -1;
    }
    Net net;
    build_net(net, (int)C_in, (int)num_classes);
    return net.count;
}

extern "C" int ps_saliency_forward(ps_context* c, const void* x, int64_t B, int64_t D, int64_t H, int64_t W, int64_t C_in, int64_t num_classes,
                                   const void* weights, int64_t weight_count, void* logits, void* probs, const ps_saliency_taps* taps, void* scratch,
                                   int64_t* scratch_bytes)
{
    return ps_saliency_forward_prec(c, x, B, D, H, W, C_in, num_classes, weights, weight_count, logits, probs, taps, scratch, scratch_bytes, PS_PREC_FP32);
}

extern "C" int ps_saliency_forward_prec(ps_context* c, const void* x, int64_t B, int64_t D, int64_t H, int64_t W, int64_t C_in, int64_t num_classes,
                                        const void* weights, int64_t weight_count, void* logits, void* probs, const ps_saliency_taps* taps,
                                        void* scratch, int64_t* scratch_bytes, int32_t precision)
{
    using namespace ps;
    const char* who = precision == PS_PREC_FP32 ? "ps_saliency_forward" : "ps_saliency_forward_prec";
    PS_CHECK(scratch_bytes && (c || !scratch), "%s: NULL argument", who);
    PS_TRY(precision_check(who, precision));
    PS_CHECK(net_args_ok(C_in, num_classes), "%s: C_in = %lld, num_classes = %lld (1 <= C_in <= 16, 2 <= num_classes <= 16)", who, (long long)C_in,
             (long long)num_classes);
    PS_CHECK(B >= 1 && B <= 1024, "%s: B = %lld, must be in [1, 1024]", who, (long long)B);
    PS_CHECK(D >= 16 && H >= 16 && W >= 16 && D % 16 == 0 && H % 16 == 0 && W % 16 == 0,
             "%s: patch %lld x %lld x %lld, every extent must be a positive multiple of 16 (four stride-2 levels)", who, (long long)D, (long long)H, (long long)W);
    PS_CHECK(D < (1 << 20) && H < (1 << 20) && W < (1 << 20) && D * H < (1ll << 31) && D * H * W * 128 < (1ll << 31),
             "%s: patch %lld x %lld x %lld, D * H * W * 128 must stay below 2^31", who, (long long)D, (long long)H, (long long)W);
    Net net;
    build_net(net, (int)C_in, (int)num_classes);
    PS_CHECK(weight_count == net.count, "%s: weight_count = %lld, the network has %lld weights", who, (long long)weight_count, (long long)net.count);

    const int nB = (int)B, K = (int)num_classes;
    int Dl[5], Hl[5], Wl[5], Vl[5];
    for (int l = 0; l < 5; ++l) Dl[l] = (int)D >> l, Hl[l] = (int)H >> l, Wl[l] = (int)W >> l, Vl[l] = Dl[l] * Hl[l] * Wl[l];
    const size_t BV0 = (size_t)nB * Vl[0];

    Carver cv{static_cast<char*>(scratch)};
    float* t0 = cv.take<float>(BV0 * 32);  // init_conv | down0_conv_0; later a spatial-attention branch's 32 channels
    float *dn[5], *ta[5], *s2[4];
    for (int d = 0; d < 5; ++d) {
        dn[d] = cv.take<float>((size_t)nB * Vl[d] * (16 << d));
        ta[d] = d ? cv.take<float>((size_t)nB * Vl[d] * (16 << d)) : t0 + BV0 * 16;
        if (d < 4) s2[d] = cv.take<float>((size_t)nB * Vl[d + 1] * (32 << d));
    }
    float* cat12 = cv.take<float>(BV0 * 128);                       // [C1 | C2 behind up_conv1_C2_up2]
    float* c2 = cv.take<float>((size_t)nB * Vl[1] * 64);
    float* cat345 = cv.take<float>((size_t)nB * Vl[2] * kCA);       // [C3_cfe | C4 | C5]
    float* cfe4 = cv.take<float>((size_t)nB * Vl[3] * 128);
    float* cfe5 = cv.take<float>((size_t)nB * Vl[4] * 128);
    float* wfold = cv.take<float>((size_t)nB * kCA * kC345);
    float* c345q = cv.take<float>((size_t)nB * Vl[2] * kC345);
    float* fuse = cv.take<float>(BV0 * 128);                        // [C12 | C345]
    float* att = cv.take<float>(BV0 * 4);                           // the three branches and their sigmoid
    float* lg = cv.take<float>(BV0 * K);
    NormWs ws;
    ws.part = cv.take<double>(norm_part_count(nB, Vl[0], kCA));
    ws.tot = cv.take<double>((size_t)nB * kCA * 2);
    ws.coef = cv.take<float2>((size_t)nB * kCA);
    if (!scratch) {
        *scratch_bytes = (int64_t)cv.off;
        return PS_OK;
    }
    PS_CHECK(x && weights, "%s: NULL x or weights (they may be NULL only in the call that sizes the scratch)", who);
    PS_CHECK(logits || probs, "%s: neither logits nor probs", who);
    PS_TRY(check_scratch(who, scratch, scratch_bytes, cv.off));

    PS_HIP(hipSetDevice(c->device));
    hipStream_t sm = c->stream;
    Stage stg(c, "saliency_forward", 200);
    const float* wt = static_cast<const float*>(weights);
    const float eps = 1e-5f;
    if (logits) lg = static_cast<float*>(logits);

    // one layer: the convolution of `in` ([B, level l's extents, cin] at pitch ldx, up-sampled `up` times) into `out` (pitch ldy), then
    // its norm + ReLU in place (+ res)
    auto layer = [&](int li, const float* in, int ldx, int l, int up, int stride, int dil, float* out, int ldy, const float* res = nullptr, int ldres = 0,
                     const float* w_over = nullptr, int64_t w_bstride = 0) {
        const Layer& L = net.L[li];
        Conv3dArgs a = {};
        a.x = in, a.x2 = nullptr, a.w = w_over ? w_over : wt + L.w, a.bias = L.b >= 0 ? wt + L.b : nullptr, a.y = out;
        a.B = nB, a.Ds = Dl[l], a.Hs = Hl[l], a.Ws = Wl[l], a.C1 = L.cin, a.C2 = 0, a.ldx = ldx, a.ldx2 = 0, a.up = up;
        a.kd = L.kd, a.kh = L.kh, a.kw = L.kw, a.cout = L.cout, a.stride = stride, a.dil = dil, a.ldy = ldy, a.w_bstride = w_bstride;
        a.precision = precision;
        conv3d_plan(a);
        conv3d_launch(sm, a);
        if (L.g >= 0) norm_run(sm, out, ldy, out, ldy, res, ldres, nB, a.Do * a.Ho * a.Wo, L.cout, wt + L.g, wt + L.be, eps, ws);
    };

    // the encoder (model.py:182-210)
    layer(net.init, static_cast<const float*>(x), (int)C_in, 0, 1, 1, 1, t0, 16);
    const float* cur = t0;
    for (int d = 0; d < 5; ++d) {
        const int w = 16 << d;
        layer(net.down[d][0], cur, w, d, 1, 1, 1, ta[d], w);
        layer(net.down[d][1], ta[d], w, d, 1, 1, 1, dn[d], w, cur, w);
        if (d < 4) {
            layer(net.s2[d], dn[d], w, d, 1, 2, 1, s2[d], 2 * w);
            cur = s2[d];
        }
    }
    if (taps && taps->down4) PS_HIP(hipMemcpyAsync(taps->down4, dn[4], (size_t)nB * Vl[4] * 256 * sizeof(float), hipMemcpyDeviceToDevice, sm));
    // the low-level features (model.py:212-228)
    layer(net.c1, dn[0], 16, 0, 1, 1, 1, cat12, 128);
    layer(net.c2, dn[1], 32, 1, 1, 1, 1, c2, 64);
    // the high-level features: CFE3D on down_list[2..4], the deeper two up-sampled to level 2 (model.py:239-251)
    float* cfe_out[3] = {cat345, cfe4, cfe5};
    const int cfe_ld[3] = {kCA, 128, 128}, rate[4] = {1, 3, 5, 7};
    for (int p = 0; p < 3; ++p)
        for (int r = 0; r < 4; ++r) layer(net.cfe[p][r], dn[2 + p], 64 << p, 2 + p, 1, 1, rate[r], cfe_out[p] + 32 * r, cfe_ld[p]);
    layer(net.up4, cfe4, 128, 3, 2, 1, 1, cat345 + 128, kCA);
    layer(net.up5, cfe5, 128, 4, 4, 1, 1, cat345 + 256, kCA);
    // the channel attention into C345_conv's kernel, C345_conv, up to full resolution (model.py:255-271)
    stats_run(sm, cat345, kCA, nB, Vl[2], kCA, ws.part, ws.tot);
    hipLaunchKernelGGL(ca_fold_kernel, dim3((unsigned)nB), dim3(256), 0, sm, ws.tot, Vl[2], wt + net.L[net.d1].w, wt + net.L[net.d1].b, wt + net.L[net.d2].w,
                       wt + net.L[net.d2].b, wt + net.L[net.c345].w, wfold);
    layer(net.c345, cat345, kCA, 2, 1, 1, 1, c345q, kC345, nullptr, 0, wfold, (int64_t)kCA * kC345);
    layer(net.up345, c345q, kC345, 2, 4, 1, 1, fuse + 64, 128);
    if (taps && taps->c345)
        hipLaunchKernelGGL(copy_rows_kernel, dim3(blocks256(BV0 * 64)), dim3(256), 0, sm, fuse + 64, 128, BV0, 64, static_cast<float*>(taps->c345));
    // the spatial attention (attention.py:79-154); t0 is free again
    for (int i = 0; i < 3; ++i) {
        layer(net.sa[i][0], fuse + 64, 128, 0, 1, 1, 1, t0, 32);
        layer(net.sa[i][1], t0, 32, 0, 1, 1, 1, att + BV0 * i, 1);
    }
    // C12 (model.py:278-295)
    layer(net.upc2, c2, 64, 1, 2, 1, 1, cat12 + 64, 128);
    layer(net.c12, cat12, 128, 0, 1, 1, 1, fuse, 128);
    float* sa = att + BV0 * 3;
    PS_TRY(gate_run(sm, att, att + BV0, att + BV0 * 2, fuse, 128, nB, Vl[0], 64, sa, fuse, 128));
    if (taps && taps->sa) PS_HIP(hipMemcpyAsync(taps->sa, sa, BV0 * sizeof(float), hipMemcpyDeviceToDevice, sm));
    if (taps && taps->c12)
        hipLaunchKernelGGL(copy_rows_kernel, dim3(blocks256(BV0 * 64)), dim3(256), 0, sm, fuse, 128, BV0, 64, static_cast<float*>(taps->c12));
    // the logits and their softmax (model.py:298-307, train.py:116)
    layer(net.fin, fuse, 128, 0, 1, 1, 1, lg, K);
    if (probs) {
        float* pr = static_cast<float*>(probs);
        const int mode = dice_mode(K, lg, pr);
        if (mode == 2) hipLaunchKernelGGL(softmax_kernel<2>, dim3(blocks256(BV0)), dim3(256), 0, sm, lg, BV0, K, pr);
        else if (mode == 4) hipLaunchKernelGGL(softmax_kernel<4>, dim3(blocks256(BV0)), dim3(256), 0, sm, lg, BV0, K, pr);
        else hipLaunchKernelGGL(softmax_kernel<1>, dim3(blocks256(BV0)), dim3(256), 0, sm, lg, BV0, K, pr);
    }
    PS_HIP(hipGetLastError());
    return PS_OK;
}

extern "C" int ps_saliency_accumulate(ps_context* c, const void* probs, int64_t p0, int64_t p1, int64_t p2, int64_t C, int64_t o0, int64_t o1, int64_t o2,
                                      int64_t D, int64_t H, int64_t W, void* sum, void* count)
{
    using namespace ps;
    static const char* who = "ps_saliency_accumulate";
    const int64_t lim = 1ll << 31;
    PS_CHECK(C >= 1 && C <= kMaxClasses, "%s: C = %lld, must be in [1, %d]", who, (long long)C, kMaxClasses);
    PS_CHECK(p0 >= 1 && p1 >= 1 && p2 >= 1 && p0 < lim && p1 < lim && p2 < lim && p0 * p1 < lim && p0 * p1 * p2 * C < lim,
             "%s: window %lld x %lld x %lld (every extent >= 1, p0 * p1 * p2 * C < 2^31)", who, (long long)p0, (long long)p1, (long long)p2);
    PS_CHECK(D >= 1 && H >= 1 && W >= 1 && D < lim && H < lim && W < lim && D * H < lim && D * H * W * C < lim,
             "%s: volume %lld x %lld x %lld (every extent >= 1, D * H * W * C < 2^31)", who, (long long)D, (long long)H, (long long)W);
    PS_CHECK(o0 >= 0 && o0 < D && o1 >= 0 && o1 < H && o2 >= 0 && o2 < W, "%s: origin (%lld, %lld, %lld) outside the volume", who, (long long)o0, (long long)o1,
             (long long)o2);
    PS_CHECK(c && probs && sum && count, "%s: NULL argument", who);
    const int n0 = (int)std::min(p0, D - o0), n1 = (int)std::min(p1, H - o1), n2 = (int)std::min(p2, W - o2);
    PS_HIP(hipSetDevice(c->device));
    Stage stg(c, "saliency_accumulate", 1);
    hipLaunchKernelGGL(window_add_kernel, dim3(blocks256((size_t)n0 * n1 * n2 * C)), dim3(256), 0, c->stream, static_cast<const float*>(probs), (int)p1, (int)p2,
                       (int)C, n0, n1, n2, (int)o0, (int)o1, (int)o2, (int)H, (int)W, static_cast<float*>(sum), static_cast<int*>(count));
    PS_HIP(hipGetLastError());
    return PS_OK;
}

extern "C" int ps_saliency_finish(ps_context* c, const void* sum, const void* count, int64_t D, int64_t H, int64_t W, int64_t C, void* out)
{
    using namespace ps;
    static const char* who = "ps_saliency_finish";
    const int64_t lim = 1ll << 31;
    PS_CHECK(C >= 1 && C <= kMaxClasses, "%s: C = %lld, must be in [1, %d]", who, (long long)C, kMaxClasses);
    PS_CHECK(D >= 1 && H >= 1 && W >= 1 && D < lim && H < lim && W < lim && D * H < lim && D * H * W * C < lim,
             "%s: volume %lld x %lld x %lld (every extent >= 1, D * H * W * C < 2^31)", who, (long long)D, (long long)H, (long long)W);
    PS_CHECK(c && sum && count && out, "%s: NULL argument", who);
    PS_HIP(hipSetDevice(c->device));
    Stage stg(c, "saliency_finish", 1);
    const unsigned total = (unsigned)(D * H * W * C);
    hipLaunchKernelGGL(window_div_kernel, dim3(blocks256(total)), dim3(256), 0, c->stream, static_cast<const float*>(sum), static_cast<const int*>(count), total,
                       (int)C, static_cast<float*>(out));
    PS_HIP(hipGetLastError());
    return PS_OK;
}
