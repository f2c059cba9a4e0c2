// saliency_map.hip -- ps_saliency_map (include/pointseg_saliency_map.h): the saliency map of a whole volume behind one
// call.  Per view and flip pass the windows of the table (saliency_map_plan.h) are gathered straight from the resident volume, `batch` at a
// time, run through ps_saliency_forward_prec, and added in window order to a sum kept in VOLUME orientation; a combine pass per view does
// the division, the running view sum and the flip's average.  No permuted or mirrored copy of the volume or of a map exists at any time.
//
// The sagittal view's fastest axis runs along the volume's H, whose stride is W * C floats.  Both of its kernels go through an LDS tile
// over (32 h, TW w) voxels instead: the volume side is walked in rows along W, the window side in rows along the view's axis 2, and the
// tile's row pitch is odd, so that the column walk of either side meets every bank once (saliency_view.h: the tile and the view permutation).
#include "saliency.h"
#include "saliency_map_plan.h"
#include "saliency_net.h"
#include "saliency_view.h"
#include "scratch.h"
#include "../../include/pointseg_saliency_map.h"

namespace ps {

namespace {

// what the kernels of one pass share
struct MapGeom {
    int D, H, W;     // the volume
    int P0, P1, P2;  // the window, view axes
    int c1, c2;      // window origins along view axes 1 and 2 (the table's inner counts)
    int s0, s1, s2;  // steps
    int flip;
};

__device__ __forceinline__ void window_origin(const MapGeom& g, int t, int& o0, int& o1, int& o2)
{
    o2 = t % g.c2 * g.s2;
    o1 = t / g.c2 % g.c1 * g.s1;
    o0 = t / (g.c2 * g.c1) * g.s0;
}

// (to_volume<VIEW> of saliency_view.h gives the volume's (d, h, w) of the PASS: before the flip's mirror)
template <int LAYOUT>
__device__ __forceinline__ float volume_at(const float* __restrict__ vol, const MapGeom& g, int C, int d, int h, int w, int c)
{
    if ((unsigned)d >= (unsigned)g.D || (unsigned)h >= (unsigned)g.H || (unsigned)w >= (unsigned)g.W) return 0.f;  // the overhang
    if (g.flip) w = g.W - 1 - w;
    const size_t vox = ((size_t)d * g.H + h) * g.W + w;
    return LAYOUT == PS_VOLUME_DHWC ? vol[vox * C + c] : vol[(size_t)c * g.D * g.H * g.W + vox];
}

// ---- window gather, axial and coronal: the window's fastest axis is the volume's W.  One lane per 16 bytes of the window. -----------------------
template <int VIEW, int LAYOUT>
__global__ __launch_bounds__(256) void map_gather_kernel(const float* __restrict__ vol, MapGeom g, int C, int t0, size_t units, float4* __restrict__ x)
{
    const size_t u = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= units) return;
    const int row4 = g.P2 * C / 4;
    const int q0 = (int)(u % row4) * 4;
    size_t r = u / row4;
    const int j = (int)(r % g.P1);
    r /= g.P1;
    const int i = (int)(r % g.P0), b = (int)(r / g.P0);
    int o0, o1, o2;
    window_origin(g, t0 + b, o0, o1, o2);
    float v[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        const int k = (q0 + n) / C, c = (q0 + n) - k * C;
        int d, h, w;
        to_volume<VIEW>(o0 + i, o1 + j, o2 + k, d, h, w);
        v[n] = volume_at<LAYOUT>(vol, g, C, d, h, w, c);
    }
    x[u] = make_float4(v[0], v[1], v[2], v[3]);
}

// ---- window gather, sagittal: window[b, i, j, k, c] = vol[d = o1 + j, h = o2 + k, w = o0 + i, c].  A workgroup owns one (b, j) and a tile of
// TW i by 32 k; grid (b * P1 + j, tiles along i, tiles along k). -----------------------------------------------------------------------------------
template <int LAYOUT>
__global__ __launch_bounds__(256) void map_gather_sagittal_kernel(const float* __restrict__ vol, MapGeom g, int C, int TW, int t0, float* __restrict__ x)
{
    __shared__ float tile[kTileH * (kTileFloats + 1)];
    const int S = (TW * C) | 1, rowf = TW * C;
    const int k0 = blockIdx.z * kTileH, i0 = blockIdx.y * TW, j = blockIdx.x % g.P1, b = blockIdx.x / g.P1;
    int o0, o1, o2;
    window_origin(g, t0 + b, o0, o1, o2);
    for (int r = threadIdx.x; r < kTileH * rowf; r += 256) {
        const int kk = r / rowf, rem = r - kk * rowf;
        int ii, c;  // the lanes run along W: voxel by voxel in the channels-last volume, within one channel plane in the other
        if (LAYOUT == PS_VOLUME_DHWC) ii = rem / C, c = rem - ii * C;
        else c = rem / TW, ii = rem - c * TW;
        float val = 0.f;
        if (i0 + ii < g.P0 && k0 + kk < g.P2) val = volume_at<LAYOUT>(vol, g, C, o1 + j, o2 + k0 + kk, o0 + i0 + ii, c);
        tile[kk * S + ii * C + c] = val;
    }
    __syncthreads();
    const int run4 = kTileH * C / 4;  // 16-byte units of one i's run over (k, c)
    for (int r = threadIdx.x; r < TW * run4; r += 256) {
        const int ii = r / run4, q0 = (r - ii * run4) * 4;
        if (i0 + ii >= g.P0 || k0 + q0 / C >= g.P2) continue;  // (P2 - k0) * C is a multiple of 4: a unit is inside or outside as a whole
        float v[4];
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const int kk = (q0 + n) / C, c = (q0 + n) - kk * C;
            v[n] = tile[kk * S + ii * C + c];
        }
        float* dst = x + ((((size_t)b * g.P0 + i0 + ii) * g.P1 + j) * g.P2 + k0) * C + q0;
        *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
    }
}

// ---- window add, axial and coronal: one launch per window, one lane per float of the part inside the volume ------------------------------------------
template <int VIEW>
__global__ __launch_bounds__(256) void map_add_kernel(const float* __restrict__ probs, MapGeom g, int K, int n0, int n1, int n2, int o0, int o1, int o2,
                                                      float* __restrict__ sum, int* __restrict__ count)
{
    const unsigned e = blockIdx.x * 256u + threadIdx.x;
    if (e >= (unsigned)n0 * n1 * n2 * K) return;
    const unsigned c = e % K, vox = e / K;
    const unsigned k = vox % n2, j = vox / n2 % n1, i = vox / (n2 * n1);
    int d, h, w;
    to_volume<VIEW>(o0 + i, o1 + j, o2 + k, d, h, w);
    if (g.flip) w = g.W - 1 - w;
    const size_t dst = ((size_t)d * g.H + h) * g.W + w;
    sum[dst * K + c] += probs[(((size_t)i * g.P1 + j) * g.P2 + k) * K + c];
    if (c == 0) count[dst] += 1;
}

// ---- window add, sagittal: sum[d = o1 + j, h = o2 + k, w = o0 + i, :] += probs[i, j, k, :] through the same tile, the other way round ---------------
__global__ __launch_bounds__(256) void map_add_sagittal_kernel(const float* __restrict__ probs, MapGeom g, int K, int TW, int n0, int n1, int n2, int o0, int o1,
                                                               int o2, float* __restrict__ sum, int* __restrict__ count)
{
    __shared__ float tile[kTileH * (kTileFloats + 1)];
    const int S = (TW * K) | 1, rowf = TW * K, runf = kTileH * K;
    const int k0 = blockIdx.z * kTileH, i0 = blockIdx.y * TW, j = blockIdx.x;
    for (int r = threadIdx.x; r < TW * runf; r += 256) {
        const int ii = r / runf, rem = r - ii * runf, kk = rem / K, c = rem - kk * K;
        if (i0 + ii < n0 && k0 + kk < n2) tile[kk * S + ii * K + c] = probs[(((size_t)(i0 + ii) * g.P1 + j) * g.P2 + k0) * K + rem];
    }
    __syncthreads();
    for (int r = threadIdx.x; r < kTileH * rowf; r += 256) {
        const int kk = r / rowf, rem = r - kk * rowf, ii = rem / K, c = rem - ii * K;
        if (i0 + ii >= n0 || k0 + kk >= n2) continue;
        int w = o0 + i0 + ii;
        if (g.flip) w = g.W - 1 - w;
        const size_t dst = ((size_t)(o1 + j) * g.H + (o2 + k0 + kk)) * g.W + w;
        sum[dst * K + c] += tile[kk * S + ii * K + c];
        if (c == 0) count[dst] += 1;
    }
}

// ---- combine, once per pass: m = sum / count; the view sum in the order of `views`; its division; the flip's average ----------------------------------
__global__ __launch_bounds__(256) void map_combine_kernel(const float* __restrict__ sum, const int* __restrict__ count, unsigned total, int K, int first, int last,
                                                          int n_views, int flip_pass, float* __restrict__ run, float* __restrict__ out)
{
    const unsigned e = blockIdx.x * 256u + threadIdx.x;
    if (e >= total) return;
    const int n = count[e / K];
    float t = n > 0 ? sum[e] / (float)n : 0.f;
    if (!first) t = run[e] + t;
    if (!last) {
        run[e] = t;
        return;
    }
    if (n_views > 1) t = t / (float)n_views;
    out[e] = flip_pass ? (out[e] + t) * 0.5f : t;
}

template <int VIEW>
void gather_launch(hipStream_t sm, int layout, const float* vol, const MapGeom& g, int C, int t0, int nb, float* x)
{
    const size_t units = (size_t)nb * g.P0 * g.P1 * g.P2 * C / 4;
    if (layout == PS_VOLUME_DHWC)
        hipLaunchKernelGGL((map_gather_kernel<VIEW, PS_VOLUME_DHWC>), dim3(blocks256(units)), dim3(256), 0, sm, vol, g, C, t0, units, reinterpret_cast<float4*>(x));
    else
        hipLaunchKernelGGL((map_gather_kernel<VIEW, PS_VOLUME_CDHW>), dim3(blocks256(units)), dim3(256), 0, sm, vol, g, C, t0, units, reinterpret_cast<float4*>(x));
}

}  // namespace

}  // namespace ps

extern "C" int ps_saliency_map(ps_context* c, const void* volume, int32_t layout, int64_t C_in, int64_t D, int64_t H, int64_t W, int64_t num_classes,
                               int32_t n_views, const int32_t* views, const void* const* weights, int64_t weight_count, const int64_t* patch,
                               const int64_t* step, int32_t flip, int32_t batch, int32_t precision, void* out, void* scratch, int64_t* scratch_bytes)
{
    using namespace ps;
    static const char* who = "ps_saliency_map";
    const int64_t lim = 1ll << 31;
    PS_CHECK(scratch_bytes && views && patch && step && (c || !scratch), "%s: NULL argument", who);
    PS_CHECK(layout == PS_VOLUME_CDHW || layout == PS_VOLUME_DHWC, "%s: layout = %d, must be PS_VOLUME_CDHW (0) or PS_VOLUME_DHWC (1)", who, (int)layout);
    PS_CHECK(n_views >= 1 && n_views <= 3, "%s: n_views = %d, must be in [1, 3]", who, (int)n_views);
    for (int v = 0; v < n_views; ++v) {
        PS_CHECK(views[v] >= PS_VIEW_AXIAL && views[v] <= PS_VIEW_CORONAL, "%s: views[%d] = %d, must be a PS_VIEW_* value (0, 1, 2)", who, v, (int)views[v]);
        for (int u = 0; u < v; ++u) PS_CHECK(views[u] != views[v], "%s: view %d is given twice", who, (int)views[v]);
    }
    PS_CHECK(flip == 0 || flip == 1, "%s: flip = %d, must be 0 or 1", who, (int)flip);
    PS_CHECK(batch >= 1 && batch <= 8, "%s: batch = %d, must be in [1, 8]", who, (int)batch);
    PS_TRY(precision_check(who, precision));
    PS_CHECK(net_args_ok(C_in, num_classes), "%s: C_in = %lld, num_classes = %lld (1 <= C_in <= 16, 2 <= num_classes <= 16)", who, (long long)C_in,
             (long long)num_classes);
    Net net;
    build_net(net, (int)C_in, (int)num_classes);
    PS_CHECK(weight_count == net.count, "%s: weight_count = %lld, the network has %lld weights", who, (long long)weight_count, (long long)net.count);
    for (int a = 0; a < 3; ++a) {
        PS_CHECK(patch[a] >= 16 && patch[a] % 16 == 0 && patch[a] < (1 << 20), "%s: patch[%d] = %lld, must be a positive multiple of 16", who, a, (long long)patch[a]);
        PS_CHECK(step[a] >= 1 && step[a] < lim, "%s: step[%d] = %lld, must be at least 1", who, a, (long long)step[a]);
    }
    PS_CHECK(patch[0] * patch[1] < lim && patch[0] * patch[1] * patch[2] * 128 < lim, "%s: patch %lld x %lld x %lld, P0 * P1 * P2 * 128 must stay below 2^31", who,
             (long long)patch[0], (long long)patch[1], (long long)patch[2]);
    PS_CHECK(D >= 1 && H >= 1 && W >= 1 && D < lim && H < lim && W < lim && D * H < lim && D * H * W * std::max(C_in, num_classes) < lim,
             "%s: volume %lld x %lld x %lld (every extent >= 1, D * H * W * max(C_in, num_classes) < 2^31)", who, (long long)D, (long long)H, (long long)W);

    MapPlan plan;
    for (int v = 0; v < n_views; ++v) {
        map_windows(views[v], D, H, W, patch, step, plan);
        PS_CHECK(plan.windows < lim, "%s: %lld windows in view %d, must stay below 2^31", who, (long long)plan.windows, (int)views[v]);
        for (int a = 0; a < 3; ++a)  // (a long step can put the last origin far behind the volume; the kernels index with int)
            PS_CHECK((plan.cnt[a] - 1) * step[a] + patch[a] < lim, "%s: step[%d] = %lld puts a window's end at or above 2^31 in view %d", who, a, (long long)step[a],
                     (int)views[v]);
    }
    int64_t fwd_bytes = 0;
    PS_TRY(ps_saliency_forward_prec(nullptr, nullptr, batch, patch[0], patch[1], patch[2], C_in, num_classes, nullptr, weight_count, nullptr, nullptr, nullptr,
                                    nullptr, &fwd_bytes, precision));
    map_scratch(D, H, W, C_in, num_classes, n_views, patch, batch, (size_t)fwd_bytes, plan);
    if (!scratch) {
        *scratch_bytes = (int64_t)plan.total;
        return PS_OK;
    }
    PS_CHECK(volume && out && weights, "%s: NULL volume, out or weights (they may be NULL only in the call that sizes the scratch)", who);
    for (int v = 0; v < n_views; ++v) PS_CHECK(weights[v], "%s: weights[%d] is NULL", who, v);
    PS_TRY(check_scratch(who, scratch, scratch_bytes, plan.total));

    PS_HIP(hipSetDevice(c->device));
    hipStream_t sm = c->stream;
    char* base = static_cast<char*>(scratch);
    float* sum = reinterpret_cast<float*>(base + plan.sum);
    float* run = reinterpret_cast<float*>(base + plan.run);
    int* count = reinterpret_cast<int*>(base + plan.count);
    float* x = reinterpret_cast<float*>(base + plan.x);
    float* probs = reinterpret_cast<float*>(base + plan.probs);
    const float* vol = static_cast<const float*>(volume);
    const int C = (int)C_in, K = (int)num_classes;
    const size_t win = (size_t)patch[0] * patch[1] * patch[2];
    const unsigned total = (unsigned)(D * H * W * K);

    for (int f = 0; f <= flip; ++f)
        for (int v = 0; v < n_views; ++v) {
            const int view = views[v];
            map_windows(view, D, H, W, patch, step, plan);
            MapGeom g;
            g.D = (int)D, g.H = (int)H, g.W = (int)W, g.P0 = (int)patch[0], g.P1 = (int)patch[1], g.P2 = (int)patch[2];
            g.c1 = (int)plan.cnt[1], g.c2 = (int)plan.cnt[2], g.s0 = (int)step[0], g.s1 = (int)step[1], g.s2 = (int)step[2], g.flip = f;
            PS_HIP(hipMemsetAsync(sum, 0, plan.map_bytes, sm));
            PS_HIP(hipMemsetAsync(count, 0, plan.count_bytes, sm));
            for (int64_t t0 = 0; t0 < plan.windows; t0 += batch) {
                const int nb = (int)std::min<int64_t>(batch, plan.windows - t0);
                {
                    Stage stg(c, "saliency_map_gather", 1);
                    if (view == kViewAxial) gather_launch<kViewAxial>(sm, layout, vol, g, C, (int)t0, nb, x);
                    else if (view == kViewCoronal) gather_launch<kViewCoronal>(sm, layout, vol, g, C, (int)t0, nb, x);
                    else {
                        const int TW = tile_w(C);
                        const dim3 grid((unsigned)(nb * g.P1), (unsigned)ceil_div(g.P0, TW), (unsigned)ceil_div(g.P2, kTileH));
                        if (layout == PS_VOLUME_DHWC)
                            hipLaunchKernelGGL(map_gather_sagittal_kernel<PS_VOLUME_DHWC>, grid, dim3(256), 0, sm, vol, g, C, TW, (int)t0, x);
                        else hipLaunchKernelGGL(map_gather_sagittal_kernel<PS_VOLUME_CDHW>, grid, dim3(256), 0, sm, vol, g, C, TW, (int)t0, x);
                    }
                }
                int64_t fb = fwd_bytes;
                PS_TRY(ps_saliency_forward_prec(c, x, nb, patch[0], patch[1], patch[2], C_in, num_classes, weights[v], weight_count, nullptr, probs, nullptr,
                                                base + plan.fwd, &fb, precision));
                Stage stg(c, "saliency_map_add", nb);
                for (int b = 0; b < nb; ++b) {  // in window order: the float32 additions of a voxel happen in the order of the table
                    int64_t o[3];
                    map_window_origin(plan, t0 + b, o);
                    const int n0 = (int)std::min(patch[0], plan.n[0] - o[0]), n1 = (int)std::min(patch[1], plan.n[1] - o[1]),
                              n2 = (int)std::min(patch[2], plan.n[2] - o[2]);
                    if (n0 <= 0 || n1 <= 0 || n2 <= 0) continue;  // step > patch can put the last origin behind the volume: numpy's empty slice
                    const float* p = probs + (size_t)b * win * K;
                    const unsigned blocks = blocks256((size_t)n0 * n1 * n2 * K);
                    if (view == kViewAxial)
                        hipLaunchKernelGGL(map_add_kernel<kViewAxial>, dim3(blocks), dim3(256), 0, sm, p, g, K, n0, n1, n2, (int)o[0], (int)o[1], (int)o[2], sum, count);
                    else if (view == kViewCoronal)
                        hipLaunchKernelGGL(map_add_kernel<kViewCoronal>, dim3(blocks), dim3(256), 0, sm, p, g, K, n0, n1, n2, (int)o[0], (int)o[1], (int)o[2], sum, count);
                    else {
                        const int TW = tile_w(K);
                        const dim3 grid((unsigned)n1, (unsigned)ceil_div(n0, TW), (unsigned)ceil_div(n2, kTileH));
                        hipLaunchKernelGGL(map_add_sagittal_kernel, grid, dim3(256), 0, sm, p, g, K, TW, n0, n1, n2, (int)o[0], (int)o[1], (int)o[2], sum, count);
                    }
                }
            }
            Stage stg(c, "saliency_map_combine", 1);
            hipLaunchKernelGGL(map_combine_kernel, dim3(blocks256(total)), dim3(256), 0, sm, sum, count, total, K, v == 0, v == n_views - 1, (int)n_views, f, run,
                               static_cast<float*>(out));
        }
    PS_HIP(hipGetLastError());
    return PS_OK;
}
