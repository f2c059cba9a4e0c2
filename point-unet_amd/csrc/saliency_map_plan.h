// saliency_map_plan.h -- the host plan of ps_saliency_map (include/pointseg_saliency_map.h): how a view's axes lie in the
// volume, the window table of one pass, and where everything lies in the caller's scratch -- functions of the shapes alone.  Host code only,
// no HIP: a plain C++ compiler takes it (asan_map_main.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

namespace ps {

enum { kViewAxial = 0, kViewSagittal = 1, kViewCoronal = 2 };

// View axis a runs along volume axis map_axis(view)[a] (0 = D, 1 = H, 2 = W):
//   axial     view[i, j, k] = vol[i, j, k]
//   sagittal  view[i, j, k] = vol[j, k, i]   np.transpose(x, (2, 0, 1)): extents (W, D, H)
//   coronal   view[i, j, k] = vol[j, i, k]   np.transpose(x, (1, 0, 2)): extents (H, D, W)
inline const int* map_axis(int view)
{
    static const int axis[3][3] = {{0, 1, 2}, {2, 0, 1}, {1, 0, 2}};
    return axis[view];
}

// eval.py:142-144: np.arange(0, max(1, n - patch + step), step) has this many values, the t-th of them t * step
inline int64_t map_origin_count(int64_t n, int64_t patch, int64_t step)
{
    const int64_t stop = n - patch + step > 1 ? n - patch + step : 1;
    return (stop + step - 1) / step;
}

struct MapPlan {
    int64_t ext[3];      // the volume's D, H, W
    int64_t n[3];        // the view's extents
    int64_t cnt[3];      // window origins per view axis
    int64_t patch[3], step[3];
    int64_t windows;     // cnt[0] * cnt[1] * cnt[2]; window t has axis 0 outermost, axis 2 innermost
    size_t sum, run, count, x, probs, fwd;  // byte offsets; run_bytes == 0 with one view
    size_t map_bytes, run_bytes, count_bytes, x_bytes, probs_bytes, fwd_bytes, total;
};

inline size_t map_pad256(size_t n) { return (n + 255) & ~(size_t)255; }

// the window table of one view
inline void map_windows(int view, int64_t D, int64_t H, int64_t W, const int64_t* patch, const int64_t* step, MapPlan& p)
{
    p.ext[0] = D, p.ext[1] = H, p.ext[2] = W;
    const int* ax = map_axis(view);
    p.windows = 1;
    for (int a = 0; a < 3; ++a) {
        p.n[a] = p.ext[ax[a]];
        p.patch[a] = patch[a], p.step[a] = step[a];
        p.cnt[a] = map_origin_count(p.n[a], patch[a], step[a]);
        p.windows *= p.cnt[a];
    }
}

// the origin of window t, in view axes
inline void map_window_origin(const MapPlan& p, int64_t t, int64_t* o)
{
    o[2] = t % p.cnt[2] * p.step[2];
    o[1] = t / p.cnt[2] % p.cnt[1] * p.step[1];
    o[0] = t / (p.cnt[2] * p.cnt[1]) * p.step[0];
}

// the scratch: ps_saliency_forward's scratch at B = batch (first, so that the forward's tensors lie as they do when the forward is called
// on a scratch of its own) | `batch` input windows [P0, P1, P2, C] | `batch` probability windows [P0, P1, P2, K] | the pass's sum
// [D, H, W, K] f32 | the running fusion [D, H, W, K] f32 (more than one view) | the count [D, H, W] i32
inline void map_scratch(int64_t D, int64_t H, int64_t W, int64_t C, int64_t K, int n_views, const int64_t* patch, int batch, size_t fwd_bytes, MapPlan& p)
{
    const size_t vox = (size_t)D * H * W, win = (size_t)patch[0] * patch[1] * patch[2];
    p.map_bytes = vox * K * sizeof(float);
    p.run_bytes = n_views > 1 ? p.map_bytes : 0;
    p.count_bytes = vox * sizeof(int32_t);
    p.x_bytes = (size_t)batch * win * C * sizeof(float);
    p.probs_bytes = (size_t)batch * win * K * sizeof(float);
    p.fwd_bytes = fwd_bytes;
    size_t off = 0;
    auto bytes = [&](size_t n) {
        const size_t at = off;
        off += map_pad256(n);
        return at;
    };
    p.fwd = bytes(p.fwd_bytes), p.x = bytes(p.x_bytes), p.probs = bytes(p.probs_bytes);
    p.sum = bytes(p.map_bytes), p.run = bytes(p.run_bytes), p.count = bytes(p.count_bytes);
    p.total = off;
}

}  // namespace ps
