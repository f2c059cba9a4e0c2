// saliency_sampler_plan.h -- the host arithmetic behind one candidate of the patch sampler (include/pointseg_saliency_data.h's rule on the
// view's extents, include/pointseg_saliency_view.h): the centre, the window, and the copied box both in VIEW axes (what the gather indexes
// a patch by) and in VOLUME axes (what the count walks).  Functions of the shapes and of the three centre hashes alone.  Host code only,
// no HIP: a plain C++ compiler takes it (asan_sampler_main.cpp).
#pragma once
#include <cstdint>

#include "saliency_map_plan.h"

namespace ps {

struct SamplerBox {
    int ext[3];   // the view's extents: ext[a] = dims[map_axis(view)[a]]
    int c[3];     // the centre, view axes
    int lo[3];    // out / 2 - r0: the box's first voxel in the patch, view axes
    int n[3];     // r0 + r1: the box's extents, view axes (0 is possible: a patch of extent 1 centred on `in`)
    int vsrc[3];  // the box's first voxel in the volume, VOLUME axes
    int vn[3];    // the box's extents, VOLUME axes: the same voxels
};

// get_random_roi_sampling_center's 'valid' branch (utils.py:390-421) with the draw replaced by the hash h: uniform on [x0, x1]
inline int sampler_centre(int in, int out, unsigned h)
{
    const int x0 = out / 2, x1 = in - x0;
    if (x1 <= x0) return (x0 + x1) / 2;
    return x0 + (int)(((unsigned long long)h * ((unsigned long long)(x1 - x0) + 1)) >> 32);  // (the span can be 2^31: not an int)
}

// dims: the volume's [d, h, w]; P: the patch in view axes; h[a]: the centre hash of view axis a
inline void sampler_box(int view, const int64_t* dims, const int64_t* P, const unsigned* h, SamplerBox& bx)
{
    const int* ax = map_axis(view);
    for (int a = 0; a < 3; ++a) {
        const int in = (int)dims[ax[a]], out = (int)P[a];
        const int ctr = sampler_centre(in, out, h[a]);
        // extract_roi_from_volume (utils.py:423-452)
        const int r0 = out / 2 < ctr ? out / 2 : ctr, r1 = out - out / 2 < in - ctr ? out - out / 2 : in - ctr;
        bx.ext[a] = in, bx.c[a] = ctr, bx.lo[a] = out / 2 - r0, bx.n[a] = r0 + r1;
        bx.vsrc[ax[a]] = ctr - r0, bx.vn[ax[a]] = r0 + r1;
    }
}

// the patch's extents as the volume's axes see them: the most the box's vn can be
inline void sampler_patch_in_volume(int view, const int64_t* P, int64_t* PV)
{
    const int* ax = map_axis(view);
    for (int a = 0; a < 3; ++a) PV[ax[a]] = P[a];
}

}  // namespace ps
