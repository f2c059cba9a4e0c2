// asan_sampler_main.cpp -- the candidate table of the patch sampler (saliency_sampler_plan.h: the centre, the window, the copied box in view
// and in volume axes) under -fsanitize=address,undefined, with no GPU and no HIP call (`make asan-sampler`;
// tests/test_saliency_view_sanitizer.py runs it and compares what it prints with the numpy restatement).
//
//     sampler_asan_check view d h w P0 P1 P2 h0 h1 h2  [the next case's ten numbers ...]
//
// Per case one line: ext[3] c[3] lo[3] n[3] vsrc[3] vn[3].  Checks on the way what the kernels rely on: the box lies inside the patch and
// inside the volume, and the volume-axes box is the view-axes one permuted.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "saliency_sampler_plan.h"

using namespace ps;

static int fail(const char* what)
{
    std::fprintf(stderr, "asan_sampler_main: %s\n", what);
    return 1;
}

int main(int argc, char** argv)
{
    if (argc < 11 || (argc - 1) % 10) return fail("usage: view d h w P0 P1 P2 h0 h1 h2, repeated");
    std::vector<long long> v;
    for (int i = 1; i < argc; ++i) v.push_back(std::strtoll(argv[i], nullptr, 10));
    for (size_t k = 0; k < v.size(); k += 10) {
        const int view = (int)v[k];
        if (view < 0 || view > 2) return fail("view out of range");
        const int64_t dims[3] = {v[k + 1], v[k + 2], v[k + 3]}, P[3] = {v[k + 4], v[k + 5], v[k + 6]};
        const unsigned h[3] = {(unsigned)v[k + 7], (unsigned)v[k + 8], (unsigned)v[k + 9]};
        for (int a = 0; a < 3; ++a)
            if (dims[a] < 1 || P[a] < 1 || dims[a] >= (1ll << 31) || P[a] >= (1ll << 31)) return fail("an extent out of range");
        SamplerBox bx;
        sampler_box(view, dims, P, h, bx);
        int64_t PV[3];
        sampler_patch_in_volume(view, P, PV);
        const int* ax = map_axis(view);
        for (int a = 0; a < 3; ++a) {
            if (bx.ext[a] != dims[ax[a]]) return fail("a view extent is not the volume's");
            if (bx.lo[a] < 0 || bx.n[a] < 0 || bx.lo[a] + bx.n[a] > P[a]) return fail("the box leaves the patch");
            if (bx.vsrc[ax[a]] < 0 || bx.vsrc[ax[a]] + bx.vn[ax[a]] > dims[ax[a]]) return fail("the box leaves the volume");
            if (bx.vn[ax[a]] != bx.n[a] || bx.vsrc[ax[a]] != bx.c[a] - (P[a] / 2 - bx.lo[a])) return fail("the volume-axes box is not the view-axes one");
            if (PV[ax[a]] != P[a] || bx.vn[ax[a]] > PV[ax[a]]) return fail("the patch in volume axes");
        }
        const int* rows[6] = {bx.ext, bx.c, bx.lo, bx.n, bx.vsrc, bx.vn};
        for (int r = 0; r < 6; ++r)
            for (int a = 0; a < 3; ++a) std::printf("%d%s", rows[r][a], r == 5 && a == 2 ? "\n" : " ");
    }
    std::printf("asan_sampler_main ok\n");
    return 0;
}
