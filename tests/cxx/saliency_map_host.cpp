// tests/cxx/saliency_map_host.cpp -- the saliency map of a whole volume from a host written against the headers ONLY (no Python, no torch):
// reads a volume and three weight buffers from a raw file, sizes the scratch, runs ps_saliency_map with the three views and the flip, and
// writes the map; tests/test_gpu_saliency_map.py compiles it with hipcc and compares the bytes with the Python call's.
//
//   saliency_map_host <in.bin> <out.bin>   in.bin: int64 header {C_in, D, H, W, num_classes, n_weights, P0, P1, P2, S0, S1, S2, batch, precision,
//                                          0, 0}, then f32 volume[C_in*D*H*W] ([C, D, H, W]), then three times f32 weights[n_weights] (axial,
//                                          sagittal, coronal);  out.bin: f32 map[D*H*W*num_classes]
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pointseg_saliency_map.h"

#define CK(expr)                                                                   \
    do {                                                                           \
        int rc_ = (expr);                                                          \
        if (rc_ != 0) {                                                            \
            std::fprintf(stderr, "%s failed: %s\n", #expr, ps_last_error());       \
            return 10;                                                             \
        }                                                                          \
    } while (0)
#define HK(expr)                                                                   \
    do {                                                                           \
        hipError_t e_ = (expr);                                                    \
        if (e_ != hipSuccess) {                                                    \
            std::fprintf(stderr, "%s failed: %s\n", #expr, hipGetErrorString(e_)); \
            return 11;                                                             \
        }                                                                          \
    } while (0)

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t h[16];
    if (std::fread(h, sizeof h, 1, f) != 1) return 3;
    const int64_t C = h[0], D = h[1], H = h[2], W = h[3], K = h[4], nw = h[5];
    const int64_t patch[3] = {h[6], h[7], h[8]}, step[3] = {h[9], h[10], h[11]};
    if (nw != ps_saliency_weight_count(C, K)) return 4;
    std::vector<float> vol((size_t)(C * D * H * W)), wts((size_t)(3 * nw));
    if (std::fread(vol.data(), 4, vol.size(), f) != vol.size() || std::fread(wts.data(), 4, wts.size(), f) != wts.size()) return 3;
    std::fclose(f);

    ps_context* ctx = nullptr;
    CK(ps_create(0, &ctx));
    float *d_vol = nullptr, *d_w = nullptr, *d_out = nullptr;
    void* d_scratch = nullptr;
    const size_t out_floats = (size_t)(D * H * W * K);
    HK(hipMalloc(&d_vol, vol.size() * 4));
    HK(hipMalloc(&d_w, wts.size() * 4));
    HK(hipMalloc(&d_out, out_floats * 4));
    HK(hipMemcpy(d_vol, vol.data(), vol.size() * 4, hipMemcpyHostToDevice));
    HK(hipMemcpy(d_w, wts.data(), wts.size() * 4, hipMemcpyHostToDevice));
    const int32_t views[3] = {PS_VIEW_AXIAL, PS_VIEW_SAGITTAL, PS_VIEW_CORONAL};
    const void* weights[3] = {d_w, d_w + nw, d_w + 2 * nw};
    int64_t need = 0;
    CK(ps_saliency_map(nullptr, nullptr, PS_VOLUME_CDHW, C, D, H, W, K, 3, views, nullptr, nw, patch, step, 1, (int32_t)h[12], (int32_t)h[13], nullptr, nullptr, &need));
    HK(hipMalloc(&d_scratch, (size_t)need));
    CK(ps_saliency_map(ctx, d_vol, PS_VOLUME_CDHW, C, D, H, W, K, 3, views, weights, nw, patch, step, 1, (int32_t)h[12], (int32_t)h[13], d_out, d_scratch, &need));
    CK(ps_synchronize(ctx));
    std::vector<float> out(out_floats);
    HK(hipMemcpy(out.data(), d_out, out_floats * 4, hipMemcpyDeviceToHost));
    FILE* g = std::fopen(argv[2], "wb");
    if (!g || std::fwrite(out.data(), 4, out.size(), g) != out.size()) return 5;
    std::fclose(g);
    std::printf("scratch_bytes %lld\n", (long long)need);
    HK(hipFree(d_scratch));
    HK(hipFree(d_out));
    HK(hipFree(d_w));
    HK(hipFree(d_vol));
    CK(ps_destroy(ctx));
    return 0;
}
