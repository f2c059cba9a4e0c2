// saliency_view.h -- the device's one statement of how an anatomical view's axes lie in a volume (saliency_map_plan.h holds the host's), and
// the LDS tile both sagittal paths go through: the window gather and add of ps_saliency_map (saliency_map.hip) and the
// patch gather of ps_patch_sample_view (saliency_data.hip).
//
// The sagittal view's fastest axis runs along the volume's H, whose stride is W * C floats.  A tile covers (32 h, TW w) voxels: the volume
// side is walked in rows along W, the view side in rows along the view's axis 2, and the tile's row pitch is odd, so that the column walk of
// either side meets every bank once.
#pragma once
#include <algorithm>

#include <hip/hip_runtime.h>

#include "saliency_map_plan.h"

namespace ps {

constexpr int kTileH = 32;        // voxels along the volume's H (the view's axis 2) in a sagittal tile
constexpr int kTileFloats = 128;  // floats of one tile row: TW voxels along W, each of E floats

inline int tile_w(int E) { return std::min(32, kTileFloats / E); }

// view voxel (v0, v1, v2) -> the volume's (d, h, w)
template <int VIEW>
__device__ __forceinline__ void to_volume(int v0, int v1, int v2, int& d, int& h, int& w)
{
    if (VIEW == kViewAxial) d = v0, h = v1, w = v2;
    else if (VIEW == kViewSagittal) w = v0, d = v1, h = v2;
    else h = v0, d = v1, w = v2;
}

}  // namespace ps
