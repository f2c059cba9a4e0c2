// saliency_data.hip -- the saliency network's data on the device (include/pointseg_saliency_data.h): the preparation of a volume
// (crop_brain_region / load_pancreas_img, SaliencyAttention/utils.py:30-78, 313-388) and training batches of patches drawn from resident
// volumes (sampler3d and BatchData's reject loop, SaliencyAttention/data_sampler.py:77-88, 169-214) by the rule the header states and
// tests/saliency_data_ref.py restates in numpy.
//
// Preparation, BraTS form: an integer min / max pass for the box of raw[0] != 0, then -- the box still on the device -- the two-pass
// statistics of every modality inside it: a float64 partial per (slab of 4096 crop voxels, modality), the threads of a slab added in a
// fixed order, the slabs by reduce_partials.h.  One copy brings the box and the sums to the host; the apply pass takes them back as arguments.
//
// Sampler: the host derives every candidate's centre and window (hashes of the seed: no device state) into one table, uploaded together
// with the zeroed counts.  Launch 1 counts the labels > 0 of the windows the mode can ask for, a row's bytes read as the aligned 4-byte
// words that cover it (the row starts at an arbitrary byte); integer atomics, so two runs agree.  Launch 2 writes the batch: every
// workgroup derives all slots' tries from the counts, then fills 16-byte pieces of the outputs -- a piece inside the copied box is loaded
// at the alignment its source address has (16, 8 or 4 bytes; labels and weights 4 or 1), a piece outside is the fill hash.
//
// Mixed batches (config.MIXUP, include/pointseg_saliency_mixup.h; tests/saliency_mixup_ref.py restates the rule): the same table and the same
// count over B + 1 drawn samples, and a gather that reads the two source windows of every output piece through the plain gather's paths,
// mixes them (two products and a sum, each rounded) and stores once -- images, the or of the weights, and the soft one-hot rows.
//
// Views and the flip (config.DIRECTION and sampler3d's np.flip, include/pointseg_saliency_view.h; tests/saliency_view_ref.py restates the
// rule): the table (saliency_sampler_plan.h) derives every candidate on the VIEW's extents and keeps its box in view and in volume axes;
// the count walks the volume-axes box as before.  The axial and coronal views' rows run along the volume's W: the two gathers above with a
// compile-time policy on the source index.  The sagittal view's rows run along H: one gather of its own through saliency_view.h's LDS
// tile, plain or mixed.  A drawn sample's flip is a bit of its table entries: the gathers read the mirrored element.  No permuted or
// mirrored copy of a volume is made.
#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

#include "common.h"
#include "reduce_partials.h"
#include "sample_hash.h"
#include "saliency_sampler_plan.h"
#include "saliency_view.h"
#include "scratch.h"
#include "wave_ops.h"

#include "../../include/pointseg_saliency_data.h"
#include "../../include/pointseg_saliency_mixup.h"
#include "../../include/pointseg_saliency_view.h"

namespace ps {

namespace {

constexpr int kCropSlab = 4096;     // crop voxels per workgroup of a statistics pass
constexpr unsigned kAxisMul = 0x85EBCA6Bu;  // h_a = hash32(s(b, t) + kAxisMul * (a + 1)); a = 3: the fill's seed

// ---- preparation ---------------------------------------------------------------------------------------------------------------------------

struct CropBox {
    int lo[3], ext[3];  // first voxel and extents (0: raw[0] is all zero)
};

// the raw min / max of raw[0] != 0 (as the box pass left them) grown by the margin and clamped
__device__ __forceinline__ CropBox crop_box(const int* __restrict__ mm, int margin, int D, int H, int W)
{
    const int dims[3] = {D, H, W};
    CropBox b;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int mn = mm[a], mx = mm[3 + a];
        if (mx < mn) {
            b.lo[a] = 0;
            b.ext[a] = 0;
        } else {
            const int l = max(mn - margin, 0), h = min(mx + margin, dims[a] - 1);
            b.lo[a] = l;
            b.ext[a] = h - l + 1;
        }
    }
    return b;
}

// crop-linear index -> the voxel's index in the uncropped volume
__device__ __forceinline__ size_t crop_source(const CropBox& b, unsigned i, int H, int W)
{
    const unsigned x = i % (unsigned)b.ext[2], r = i / (unsigned)b.ext[2];
    const unsigned y = r % (unsigned)b.ext[1], z = r / (unsigned)b.ext[1];
    return ((size_t)(b.lo[0] + z) * H + (b.lo[1] + y)) * W + (b.lo[2] + x);
}

__global__ __launch_bounds__(256) void brats_box_kernel(const float* __restrict__ raw0, unsigned nvox, int H, int W, int* __restrict__ mm)
{
    int mn[3] = {INT_MAX, INT_MAX, INT_MAX}, mx[3] = {-1, -1, -1};
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < nvox; i += gridDim.x * 256u) {
        if (raw0[i] == 0.f) continue;
        const int x = (int)(i % (unsigned)W), r = (int)(i / (unsigned)W);
        const int p[3] = {r / H, r % H, x};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            mn[a] = min(mn[a], p[a]);
            mx[a] = max(mx[a], p[a]);
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int lo = (int)wave_allreduce_u32((unsigned)mn[a], [](unsigned p, unsigned q) { return (unsigned)min((int)p, (int)q); });
        const int hi = (int)wave_allreduce_u32((unsigned)mx[a], [](unsigned p, unsigned q) { return (unsigned)max((int)p, (int)q); });
        if ((threadIdx.x & 63) == 0) {
            if (lo != INT_MAX) atomicMin(&mm[a], lo);
            if (hi >= 0) atomicMax(&mm[3 + a], hi);
        }
    }
}

// the 256 values of a workgroup added in one fixed tree; the sum is in thread 0
__device__ __forceinline__ double block_sum_fixed(double v, double* ss)
{
    ss[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) ss[threadIdx.x] += ss[threadIdx.x + s];
        __syncthreads();
    }
    return ss[0];
}

// DEV = false: part[slab][c][2] = (sum, count) of the voxels > 0; DEV = true: part[slab][c] = sum of (v - mean)^2, mean from tot.
// grid (slabs of the UNCROPPED volume, C): slabs past the crop write zeros.
template <bool DEV>
__global__ __launch_bounds__(256) void brats_stats_kernel(const float* __restrict__ raw, size_t nvox, int D, int H, int W, int margin,
                                                          const int* __restrict__ mm, const double* __restrict__ tot, double* __restrict__ part)
{
    __shared__ double ss[256];
    const CropBox b = crop_box(mm, margin, D, H, W);
    const unsigned ncrop = (unsigned)b.ext[0] * (unsigned)b.ext[1] * (unsigned)b.ext[2];
    const int c = blockIdx.y, C = gridDim.y;
    const float* v = raw + (size_t)c * nvox;
    const double mean = DEV ? tot[2 * c] / tot[2 * c + 1] : 0.0;
    double s = 0.0, n = 0.0;
    const unsigned i0 = blockIdx.x * (unsigned)kCropSlab;
    for (int u = 0; u < kCropSlab / 256; ++u) {
        const unsigned i = i0 + u * 256u + threadIdx.x;
        if (i >= ncrop) break;
        const float f = v[crop_source(b, i, H, W)];
        if (f > 0.f) {
            if (DEV) {
                const double d = (double)f - mean;
                s += d * d;
            } else {
                s += (double)f;
                n += 1.0;
            }
        }
    }
    s = block_sum_fixed(s, ss);
    if (DEV) {
        if (threadIdx.x == 0) part[(size_t)blockIdx.x * C + c] = s;
    } else {
        __syncthreads();
        n = block_sum_fixed(n, ss);
        if (threadIdx.x == 0) {
            part[((size_t)blockIdx.x * C + c) * 2] = s;
            part[((size_t)blockIdx.x * C + c) * 2 + 1] = n;
        }
    }
}

struct ApplyArgs {
    double mean[PS_PATCH_MAX_C], sd[PS_PATCH_MAX_C];
    CropBox box;
};

// one thread per crop voxel: C normalised values (channels-last), the label, the weight
__global__ __launch_bounds__(256) void brats_apply_kernel(const float* __restrict__ raw, const int32_t* __restrict__ seg, size_t nvox, int H, int W, int C,
                                                          int num_class, ApplyArgs a, unsigned ncrop, float* __restrict__ image,
                                                          uint8_t* __restrict__ label, uint8_t* __restrict__ weight)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= ncrop) return;
    const size_t src = crop_source(a.box, i, H, W);
    float* o = image + (size_t)i * C;
    for (int c = 0; c < C; ++c) {
        const float f = raw[(size_t)c * nvox + src];
        o[c] = f == 0.f ? 0.f : (float)(((double)f - a.mean[c]) / a.sd[c]);
    }
    weight[i] = raw[src] > 0.f ? 1 : 0;
    int l = seg ? seg[src] : 0;
    if (num_class == 4) l = l == 4 ? 3 : l;
    else l = (l == 4 || l == 2) ? 1 : l;
    label[i] = (uint8_t)l;
}

template <class T>
__global__ __launch_bounds__(256) void pancreas_prepare_kernel(const T* __restrict__ ct, size_t n, const uint8_t* __restrict__ label,
                                                               float* __restrict__ image, uint8_t* __restrict__ out_label, uint8_t* __restrict__ weight)
{
    for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        image[i] = (float)(((double)ct[i] + 100.0) / 340.0);
        out_label[i] = label ? label[i] : 0;
        weight[i] = 1;
    }
}

// ---- the sampler ---------------------------------------------------------------------------------------------------------------------------

// candidate (slot b, try t), host-filled (saliency_sampler_plan.h): the window of the rule, as the kernels need it.  The patch side is in
// VIEW axes, the volume side in VOLUME axes [d, h, w]; with the axial view the two are the same.
struct PatchCand {
    const float* img;
    const uint8_t* lab;
    const uint8_t* wgt;
    int dim[3];   // the volume's extents (volume axes)
    int c[3];     // the centre (view axes)
    int src[3];   // the box's first voxel in the volume (volume axes)
    int vn[3];    // the box's extents (volume axes): what the count walks
    int lo[3];    // out / 2 - r0: the box's first voxel in the patch (view axes)
    int n[3];     // r0 + r1: the box's extents (view axes; 0 is possible: a patch of extent 1 centred on `in`)
    unsigned s_fill;
    int vol;
    int count;    // its index in the counts, -1: never asked for
    int flip;     // the drawn sample's flip bit: its patch is written mirrored along the view's last axis
};

struct PatchShape {
    int P[3], C, B, T, mode;
};

// labels > 0 in bytes [a, a + len) of a volume [base, end): through the aligned words that lie inside the volume, bytes at its two ends
__device__ __forceinline__ unsigned count_word(uintptr_t q, uintptr_t a, uintptr_t a_end, uintptr_t base, uintptr_t end)
{
    const uintptr_t f = a > q ? a : q, l = a_end < q + 4 ? a_end : q + 4;
    if (f >= l) return 0;
    if (q >= base && q + 4 <= end) {
        const unsigned lo = (unsigned)(f - q), hi = (unsigned)(l - q);
        unsigned m = hi == 4 ? ~0u : (1u << (8 * hi)) - 1u;
        m &= ~((1u << (8 * lo)) - 1u);
        const unsigned x = *reinterpret_cast<const unsigned*>(q) & m;
        return (unsigned)__popc((((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u);
    }
    unsigned n = 0;
    for (uintptr_t p = f; p < l; ++p) n += *reinterpret_cast<const uint8_t*>(p) != 0;
    return n;
}

// Launch 1.  grid (blocks of 2048 words, windows); a window's rows -- along the volume's W, over the box in volume axes: a box is the same
// set of voxels in any view -- are kdw words each (the most a row of the patch's extent along W can touch).
__global__ __launch_bounds__(256) void patch_count_kernel(const PatchCand* __restrict__ cands, const int* __restrict__ win, unsigned* __restrict__ counts,
                                                          unsigned kdw)
{
    const PatchCand& cd = cands[win[blockIdx.y]];
    const unsigned rows = (unsigned)cd.vn[0] * (unsigned)cd.vn[1], total = rows * kdw;
    const unsigned i0 = blockIdx.x * 2048u;
    if (i0 >= total || cd.vn[2] == 0) return;
    const uintptr_t base = reinterpret_cast<uintptr_t>(cd.lab);
    const uintptr_t end = base + (size_t)cd.dim[0] * cd.dim[1] * cd.dim[2];
    unsigned n = 0;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const unsigned i = i0 + u * 256u + threadIdx.x;
        if (i < total) {
            const unsigned row = i / kdw, k = i - row * kdw;
            const unsigned y = row % (unsigned)cd.vn[1], z = row / (unsigned)cd.vn[1];
            const uintptr_t a = base + ((size_t)(cd.src[0] + z) * cd.dim[1] + (cd.src[1] + y)) * cd.dim[2] + cd.src[2];
            n += count_word((a & ~(uintptr_t)3) + 4 * (uintptr_t)k, a, a + cd.vn[2], base, end);
        }
    }
    n = (unsigned)wave_sum((int)n);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(&counts[cd.count], n);
}

// The rule's choice of try for slot b (thread-serial; the same in every workgroup).  any_earlier: some slot b' < B - 1 has pos(b', 0) > 0.
__device__ __forceinline__ int choose_try(const PatchCand* __restrict__ cands, const unsigned* __restrict__ counts, const PatchShape& sh, int b,
                                          bool any_earlier, int& ok)
{
    ok = 1;
    if (sh.mode == PS_PATCH_RANDOM) return 0;
    if (sh.mode == PS_PATCH_ONE_POSITIVE && (b < sh.B - 1 || any_earlier)) return 0;
    for (int t = 0; t < sh.T; ++t)
        if (counts[cands[b * sh.T + t].count] > 0) return t;
    ok = 0;
    return sh.T - 1;
}

__device__ __forceinline__ float fill_value(unsigned j, unsigned s_fill) { return (float)(point_hash(j, s_fill) >> 8) * 0x1p-24f; }

// voxel (u0, u1, u2) of the copied box, counted in VIEW axes from the box's first voxel: its index in the volume
template <int VIEW>
__device__ __forceinline__ size_t box_voxel(const PatchCand& cd, unsigned u0, unsigned u1, unsigned u2)
{
    int d, h, w;
    to_volume<VIEW>((int)u0, (int)u1, (int)u2, d, h, w);
    return ((size_t)(cd.src[0] + d) * cd.dim[1] + (cd.src[1] + h)) * cd.dim[2] + (cd.src[2] + w);
}

// element j of a slot's [P0, P1, P2, C] patch.  A flipped sample's element (.., k, c) is the unflipped one's (.., P2 - 1 - k, c), its fill
// included: the fill is keyed by the index before the flip.
template <int VIEW>
__device__ __forceinline__ float image_element(const PatchCand& cd, const PatchShape& sh, unsigned j)
{
    const unsigned c = j % (unsigned)sh.C, v = j / (unsigned)sh.C;
    unsigned p2 = v % (unsigned)sh.P[2];
    const unsigned r = v / (unsigned)sh.P[2];
    if (cd.flip) {
        p2 = (unsigned)sh.P[2] - 1u - p2;
        j = (r * (unsigned)sh.P[2] + p2) * (unsigned)sh.C + c;
    }
    const unsigned u0 = r / (unsigned)sh.P[1] - (unsigned)cd.lo[0], u1 = r % (unsigned)sh.P[1] - (unsigned)cd.lo[1], u2 = p2 - (unsigned)cd.lo[2];
    if (u0 < (unsigned)cd.n[0] && u1 < (unsigned)cd.n[1] && u2 < (unsigned)cd.n[2]) return cd.img[box_voxel<VIEW>(cd, u0, u1, u2) * sh.C + c];
    return fill_value(j, cd.s_fill);
}

// voxel v of a slot's [P0, P1, P2] patch: its index in the volume, or -1 outside the copied box
template <int VIEW>
__device__ __forceinline__ long long voxel_source(const PatchCand& cd, const PatchShape& sh, unsigned v)
{
    unsigned p2 = v % (unsigned)sh.P[2];
    const unsigned r = v / (unsigned)sh.P[2];
    if (cd.flip) p2 = (unsigned)sh.P[2] - 1u - p2;
    const unsigned u0 = r / (unsigned)sh.P[1] - (unsigned)cd.lo[0], u1 = r % (unsigned)sh.P[1] - (unsigned)cd.lo[1], u2 = p2 - (unsigned)cd.lo[2];
    if (u0 < (unsigned)cd.n[0] && u1 < (unsigned)cd.n[1] && u2 < (unsigned)cd.n[2]) return (long long)box_voxel<VIEW>(cd, u0, u1, u2);
    return -1;
}

// four image elements from e0 on (e0 % 4 == 0), of the batch's E; ROW4: P2 * C % 4 == 0, the four share a row of one slot.  VIEW is axial
// or coronal: the view's last axis is the volume's W, a patch row is one run of the source.  (A flipped sample keeps the row path where
// C % 4 == 0 -- the four are one voxel's channels -- and goes element by element elsewhere.)
template <bool ROW4, int VIEW>
__device__ __forceinline__ void image_quad(const PatchCand* s_c, const PatchShape& sh, unsigned L, size_t e0, size_t E, float (&o)[4])
{
    const unsigned b = (unsigned)(e0 / L);
    if (ROW4 && (!s_c[b].flip || (sh.C & 3) == 0)) {
        unsigned j = (unsigned)(e0 - (size_t)b * L);
        const PatchCand& cd = s_c[b];
        const unsigned rowlen = (unsigned)sh.P[2] * (unsigned)sh.C, row = j / rowlen;
        unsigned col = j - row * rowlen;
        if (cd.flip) {
            const unsigned k = col / (unsigned)sh.C;
            col = ((unsigned)sh.P[2] - 1u - k) * (unsigned)sh.C + (col - k * (unsigned)sh.C);
            j = row * rowlen + col;
        }
        const unsigned u0 = row / (unsigned)sh.P[1] - (unsigned)cd.lo[0], u1 = row % (unsigned)sh.P[1] - (unsigned)cd.lo[1];
        const unsigned lo = (unsigned)cd.lo[2] * (unsigned)sh.C, hi = lo + (unsigned)cd.n[2] * (unsigned)sh.C;
        const bool row_in = u0 < (unsigned)cd.n[0] && u1 < (unsigned)cd.n[1];
        if (row_in && col >= lo && col + 4 <= hi) {  // four consecutive floats of the source: at the alignment that address has
            const float* p = cd.img + box_voxel<VIEW>(cd, u0, u1, 0) * sh.C + (col - lo);
            const uintptr_t a = reinterpret_cast<uintptr_t>(p);
            if ((a & 15) == 0) {
                const float4 f = *reinterpret_cast<const float4*>(p);
                o[0] = f.x, o[1] = f.y, o[2] = f.z, o[3] = f.w;
            } else if ((a & 7) == 0) {
                const float2 f = *reinterpret_cast<const float2*>(p), g = *reinterpret_cast<const float2*>(p + 2);
                o[0] = f.x, o[1] = f.y, o[2] = g.x, o[3] = g.y;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) o[k] = p[k];
            }
            return;
        }
        if (!row_in || col + 4 <= lo || col >= hi) {
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = fill_value(j + k, cd.s_fill);
            return;
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const size_t e = e0 + k;
        o[k] = 0.f;
        if (e < E) {
            const unsigned be = (unsigned)(e / L);
            o[k] = image_element<VIEW>(s_c[be], sh, (unsigned)(e - (size_t)be * L));
        }
    }
}

// labels and weights of four voxels from e0 on (e0 % 4 == 0), of the batch's E = slots * V; zeros outside the copied boxes and past E
template <int VIEW>
__device__ __forceinline__ void voxel_quad(const PatchCand* s_c, const PatchShape& sh, unsigned V, size_t e0, size_t E, int (&l)[4], float (&w)[4])
{
#pragma unroll
    for (int k = 0; k < 4; ++k) l[k] = 0, w[k] = 0.f;
    if ((sh.P[2] & 3) == 0) {  // the four voxels share a row of one slot: one word each where the box holds them all and the bytes are aligned
        const unsigned b = (unsigned)(e0 / V), v = (unsigned)(e0 - (size_t)b * V);
        const PatchCand& cd = s_c[b];
        const long long s0 = voxel_source<VIEW>(cd, sh, v), s3 = voxel_source<VIEW>(cd, sh, v + 3);
        const long long sl = cd.flip ? s3 : s0;  // (a flipped sample's four lie the other way round)
        if (s0 >= 0 && s3 >= 0 && ((reinterpret_cast<uintptr_t>(cd.lab + sl) | reinterpret_cast<uintptr_t>(cd.wgt + sl)) & 3) == 0) {
            unsigned x = *reinterpret_cast<const unsigned*>(cd.lab + sl), y = *reinterpret_cast<const unsigned*>(cd.wgt + sl);
            if (cd.flip) x = __builtin_bswap32(x), y = __builtin_bswap32(y);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                l[k] = (int)((x >> (8 * k)) & 255u);
                w[k] = (float)((y >> (8 * k)) & 255u);
            }
            return;
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const size_t e = e0 + k;
        if (e >= E) break;
        const unsigned b = (unsigned)(e / V);
        const PatchCand& cd = s_c[b];
        const long long s = voxel_source<VIEW>(cd, sh, (unsigned)(e - (size_t)b * V));
        if (s >= 0) {
            l[k] = cd.lab[s];
            w[k] = (float)cd.wgt[s];
        }
    }
}

// Launch 2.  Workgroups [0, img_blocks) write 1024 quads of images each, the rest 1024 quads of labels and weights; workgroup 0 also
// writes info.  vec_i / vec_v: the image / the label and weight outputs are 16-byte aligned.
template <bool ROW4, int VIEW>
__global__ __launch_bounds__(256) void patch_gather_kernel(const PatchCand* __restrict__ cands, const unsigned* __restrict__ counts, PatchShape sh,
                                                           unsigned img_blocks, bool vec_i, bool vec_v, float* __restrict__ out_i,
                                                           float* __restrict__ out_w, int32_t* __restrict__ out_l, int32_t* __restrict__ info)
{
    __shared__ PatchCand s_c[PS_PATCH_MAX_B];
    const int t = threadIdx.x;
    bool pos0 = false;
    if (sh.mode == PS_PATCH_ONE_POSITIVE && t < sh.B - 1) pos0 = counts[cands[t * sh.T].count] > 0;
    const bool any_earlier = __syncthreads_or(pos0) != 0;
    if (t < sh.B) {
        int ok;
        const int tr = choose_try(cands, counts, sh, t, any_earlier, ok);
        const PatchCand cd = cands[t * sh.T + tr];
        s_c[t] = cd;
        if (blockIdx.x == 0) {
            int32_t* r = info + 8 * t;
            r[0] = tr, r[1] = cd.vol, r[2] = cd.c[0], r[3] = cd.c[1], r[4] = cd.c[2], r[5] = (int32_t)counts[cd.count], r[6] = ok, r[7] = cd.flip;
        }
    }
    __syncthreads();
    const unsigned V = (unsigned)sh.P[0] * (unsigned)sh.P[1] * (unsigned)sh.P[2], L = V * (unsigned)sh.C;
    if (blockIdx.x < img_blocks) {
        const size_t E = (size_t)sh.B * L;
#pragma unroll 2
        for (int u = 0; u < 4; ++u) {
            const size_t e0 = 4 * ((size_t)blockIdx.x * 1024 + u * 256 + t);
            if (e0 >= E) break;
            float o[4];
            image_quad<ROW4, VIEW>(s_c, sh, L, e0, E, o);
            if (vec_i && e0 + 4 <= E) {
                *reinterpret_cast<float4*>(out_i + e0) = make_float4(o[0], o[1], o[2], o[3]);
            } else {
                for (int k = 0; k < 4; ++k)
                    if (e0 + k < E) out_i[e0 + k] = o[k];
            }
        }
        return;
    }
    const size_t E = (size_t)sh.B * V;
    for (int u = 0; u < 4; ++u) {
        const size_t e0 = 4 * ((size_t)(blockIdx.x - img_blocks) * 1024 + u * 256 + t);
        if (e0 >= E) break;
        int l[4];
        float w[4];
        voxel_quad<VIEW>(s_c, sh, V, e0, E, l, w);
        if (vec_v && e0 + 4 <= E) {
            *reinterpret_cast<int4*>(out_l + e0) = make_int4(l[0], l[1], l[2], l[3]);
            *reinterpret_cast<float4*>(out_w + e0) = make_float4(w[0], w[1], w[2], w[3]);
        } else {
            for (int k = 0; k < 4; ++k)
                if (e0 + k < E) {
                    out_l[e0 + k] = l[k];
                    out_w[e0 + k] = w[k];
                }
        }
    }
}

// ---- the mixed gather (include/pointseg_saliency_mixup.h) ----------------------------------------------------------------------------------------

// The mixed batch's choice of try for DRAWN sample i of sh.B + 1 (thread-serial; the same in every workgroup): the reject loop's check
// fires on sample sh.B - 1, the last sample is free.  any_earlier: some sample i' < sh.B - 1 has pos(i', 0) > 0.
__device__ __forceinline__ int choose_try_mixup(const PatchCand* __restrict__ cands, const unsigned* __restrict__ counts, const PatchShape& sh, int i,
                                                bool any_earlier, int& ok)
{
    ok = 1;
    if (sh.mode == PS_PATCH_RANDOM) return 0;
    if (sh.mode == PS_PATCH_ONE_POSITIVE && (i != sh.B - 1 || any_earlier)) return 0;
    for (int t = 0; t < sh.T; ++t)
        if (counts[cands[i * sh.T + t].count] > 0) return t;
    ok = 0;
    return sh.T - 1;
}

// fl32(fl32(g * a) + fl32(h * b)): mixup's rule (utils.py:523, 525), every product and the sum rounded on its own
__device__ __forceinline__ float mix(float2 gh, float a, float b) { return __fadd_rn(__fmul_rn(gh.x, a), __fmul_rn(gh.y, b)); }

// The slots of the four elements from e0 on, `len` elements to a slot, clamped to `last` (an element past the batch's end is never stored).
// same: the four share a slot.  One 64-bit division, the one the quad readers make as well; the rest is 32-bit.
__device__ __forceinline__ void quad_slots(size_t e0, unsigned len, bool same, unsigned last, unsigned (&b)[4])
{
    const unsigned b0 = (unsigned)(e0 / len), j = (unsigned)(e0 - (size_t)b0 * len);
#pragma unroll
    for (int k = 0; k < 4; ++k) b[k] = same ? b0 : min(last, b0 + (j + k) / len);
}

// class c of the mixed one-hot rows of labels l1 and l2
__device__ __forceinline__ float mix_class(float2 gh, int l1, int l2, int c) { return mix(gh, l1 == c ? 1.f : 0.f, l2 == c ? 1.f : 0.f); }

// Launch 2 of the mixed batch: patch_gather_kernel's partition over sh.B MIXED slots.  s_c holds the sh.B + 1 drawn samples, so slot b's
// two sources are s_c[b] and (s_c + 1)[b]: every piece is read twice through the plain gather's paths, mixed, and stored once.  gh[b] =
// (float32(gamma_b), float32(1 - gamma_b)).  The soft rows are written along K: two rows in one 16-byte store for K == 2, 16 bytes at a
// time for K % 4 == 0 (both where out_s is 16-byte aligned: al_s >= 16), 8 bytes for another even K (al_s >= 8), floats elsewhere.
// (__launch_bounds__(256, 8): the plain gather's 8 waves per SIMD -- 63 registers, nothing spilled; left alone the compiler takes 68.)
template <bool ROW4, int VIEW>
__global__ __launch_bounds__(256, 8) void patch_mix_kernel(const PatchCand* __restrict__ cands, const unsigned* __restrict__ counts,
                                                        const float2* __restrict__ gh, PatchShape sh, int K, unsigned img_blocks, bool vec_i, bool vec_w,
                                                        int al_s, float* __restrict__ out_i, float* __restrict__ out_w, float* __restrict__ out_s,
                                                        int32_t* __restrict__ info)
{
    __shared__ PatchCand s_c[PS_PATCH_MAX_B];
    __shared__ float2 s_g[PS_PATCH_MAX_B];
    const int t = threadIdx.x;
    bool pos0 = false;
    if (sh.mode == PS_PATCH_ONE_POSITIVE && t < sh.B - 1) pos0 = counts[cands[t * sh.T].count] > 0;
    const bool any_earlier = __syncthreads_or(pos0) != 0;
    if (t <= sh.B) {
        int ok;
        const int tr = choose_try_mixup(cands, counts, sh, t, any_earlier, ok);
        const PatchCand cd = cands[t * sh.T + tr];
        s_c[t] = cd;
        if (t < sh.B) s_g[t] = gh[t];
        if (blockIdx.x == 0) {
            int32_t* r = info + 8 * t;
            r[0] = tr, r[1] = cd.vol, r[2] = cd.c[0], r[3] = cd.c[1], r[4] = cd.c[2], r[5] = (int32_t)counts[cd.count], r[6] = ok, r[7] = cd.flip;
        }
    }
    __syncthreads();
    const unsigned V = (unsigned)sh.P[0] * (unsigned)sh.P[1] * (unsigned)sh.P[2], L = V * (unsigned)sh.C;
    if (blockIdx.x < img_blocks) {
        const size_t E = (size_t)sh.B * L;
#pragma unroll 2
        for (int u = 0; u < 4; ++u) {
            const size_t e0 = 4 * ((size_t)blockIdx.x * 1024 + u * 256 + t);
            if (e0 >= E) break;
            float a[4], b[4], o[4];
            unsigned slot[4];
            image_quad<ROW4, VIEW>(s_c, sh, L, e0, E, a);
            image_quad<ROW4, VIEW>(s_c + 1, sh, L, e0, E, b);
            quad_slots(e0, L, ROW4, (unsigned)sh.B - 1, slot);
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = mix(s_g[slot[k]], a[k], b[k]);
            if (vec_i && e0 + 4 <= E) {
                *reinterpret_cast<float4*>(out_i + e0) = make_float4(o[0], o[1], o[2], o[3]);
            } else {
                for (int k = 0; k < 4; ++k)
                    if (e0 + k < E) out_i[e0 + k] = o[k];
            }
        }
        return;
    }
    const size_t E = (size_t)sh.B * V;
#pragma unroll 1
    for (int u = 0; u < 4; ++u) {
        const size_t e0 = 4 * ((size_t)(blockIdx.x - img_blocks) * 1024 + u * 256 + t);
        if (e0 >= E) break;
        // (the two samples' labels as four bytes each and their weights as the or's bits: what stays in registers across the stores)
        unsigned lp1 = 0, lp2 = 0, wm = 0;
        {
            int l[4];
            float w[4];
            voxel_quad<VIEW>(s_c, sh, V, e0, E, l, w);
#pragma unroll
            for (int k = 0; k < 4; ++k) lp1 |= (unsigned)l[k] << (8 * k), wm |= (w[k] != 0.f ? 1u : 0u) << k;
            voxel_quad<VIEW>(s_c + 1, sh, V, e0, E, l, w);
#pragma unroll
            for (int k = 0; k < 4; ++k) lp2 |= (unsigned)l[k] << (8 * k), wm |= (w[k] != 0.f ? 1u : 0u) << k;
        }
        const bool full = e0 + 4 <= E;
        if (vec_w && full) {
            *reinterpret_cast<float4*>(out_w + e0) = make_float4(wm & 1u ? 1.f : 0.f, wm & 2u ? 1.f : 0.f, wm & 4u ? 1.f : 0.f, wm & 8u ? 1.f : 0.f);
        } else {
            for (int k = 0; k < 4; ++k)
                if (e0 + k < E) out_w[e0 + k] = (wm >> k) & 1u ? 1.f : 0.f;
        }
        const unsigned v0 = (unsigned)e0;  // (B * V * K < 2^31)
        unsigned slot[4];
        quad_slots(e0, V, (sh.P[2] & 3) == 0, (unsigned)sh.B - 1, slot);
        if (K == 2 && al_s >= 16 && full) {
#pragma unroll
            for (int k = 0; k < 4; k += 2) {
                const float2 ga = s_g[slot[k]], gb = s_g[slot[k + 1]];
                const int a1 = (int)((lp1 >> (8 * k)) & 255u), a2 = (int)((lp2 >> (8 * k)) & 255u);
                const int b1 = (int)((lp1 >> (8 * k + 8)) & 255u), b2 = (int)((lp2 >> (8 * k + 8)) & 255u);
                *reinterpret_cast<float4*>(out_s + (size_t)(v0 + k) * 2) =
                    make_float4(mix_class(ga, a1, a2, 0), mix_class(ga, a1, a2, 1), mix_class(gb, b1, b2, 0), mix_class(gb, b1, b2, 1));
            }
            continue;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (e0 + k >= E) break;
            const float2 g = s_g[slot[k]];
            const int l1 = (int)((lp1 >> (8 * k)) & 255u), l2 = (int)((lp2 >> (8 * k)) & 255u);
            float* o = out_s + (size_t)(v0 + k) * K;
            if ((K & 3) == 0 && al_s >= 16) {
                for (int c = 0; c < K; c += 4)
                    *reinterpret_cast<float4*>(o + c) = make_float4(mix_class(g, l1, l2, c), mix_class(g, l1, l2, c + 1), mix_class(g, l1, l2, c + 2),
                                                                     mix_class(g, l1, l2, c + 3));
            } else if ((K & 1) == 0 && al_s >= 8) {
                for (int c = 0; c < K; c += 2) *reinterpret_cast<float2*>(o + c) = make_float2(mix_class(g, l1, l2, c), mix_class(g, l1, l2, c + 1));
            } else {
                for (int c = 0; c < K; ++c) o[c] = mix_class(g, l1, l2, c);
            }
        }
    }
}

// ---- the sagittal gather (include/pointseg_saliency_view.h) --------------------------------------------------------------------
// patch[i, j, k, c] = vol[d = j, h = k, w = i, c]: the patch's rows run along the volume's H, whose stride is W * C floats.  A workgroup
// owns one (slot b, view row j) and a tile of TW view-i by 32 view-k OUTPUT voxels; grid (b * P1 + j, tiles along i, tiles along k).  The
// volume side is read in rows along W into an LDS tile of odd pitch (saliency_view.h), the patch side is written in rows along k.  What
// lies outside the copied box is never staged: the write side takes the fill hash of the element's patch index (before the flip) there.
// A flipped sample's tile holds source k in [P2 - k1, P2 - k0) for the output's [k0, k1).  MIX: both drawn samples of slot b are staged,
// each with its own box and flip, mixed by mix() / mix_class() and stored once.  Labels and weights then go through the same tile, a voxel
// packed as label | weight << 8.  vec_i / vec_v: 16-byte stores of images / of labels and weights (the rows' lengths and the outputs'
// addresses allow them); the soft rows are written as floats, consecutive lanes on consecutive addresses.

// the tile's source range along k of one sample, and whether row j of the patch meets its box
struct SagittalRow {
    int ks0;
    bool in;
};

template <bool MIX>
__global__ __launch_bounds__(256) void patch_gather_sagittal_kernel(const PatchCand* __restrict__ cands, const unsigned* __restrict__ counts,
                                                                    const float2* __restrict__ gh, PatchShape sh, int K, int TW, bool vec_i, bool vec_v,
                                                                    float* __restrict__ out_i, float* __restrict__ out_w, int32_t* __restrict__ out_l,
                                                                    float* __restrict__ out_s, int32_t* __restrict__ info)
{
    constexpr int NS = MIX ? 2 : 1;
    __shared__ float tile[NS][kTileH * (kTileFloats + 1)];
    __shared__ PatchCand s_c[NS];
    __shared__ float2 s_g;
    const int t = threadIdx.x;
    const int P0 = sh.P[0], P1 = sh.P[1], P2 = sh.P[2], C = sh.C;
    const int b = (int)(blockIdx.x / (unsigned)P1), j = (int)(blockIdx.x - (unsigned)b * (unsigned)P1);
    const int i0 = blockIdx.y * TW, k0 = blockIdx.z * kTileH, k1 = min(k0 + kTileH, P2);
    bool pos0 = false;
    if (sh.mode == PS_PATCH_ONE_POSITIVE && t < sh.B - 1) pos0 = counts[cands[t * sh.T].count] > 0;
    const bool any_earlier = __syncthreads_or(pos0) != 0;
    if (t < sh.B + (MIX ? 1 : 0)) {
        int ok;
        const int tr = MIX ? choose_try_mixup(cands, counts, sh, t, any_earlier, ok) : choose_try(cands, counts, sh, t, any_earlier, ok);
        const PatchCand cd = cands[t * sh.T + tr];
        if (t == b) s_c[0] = cd;
        if (MIX && t == b + 1) s_c[NS - 1] = cd;
        if (MIX && t == b) s_g = gh[b];
        if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0) {
            int32_t* r = info + 8 * t;
            r[0] = tr, r[1] = cd.vol, r[2] = cd.c[0], r[3] = cd.c[1], r[4] = cd.c[2], r[5] = (int32_t)counts[cd.count], r[6] = ok, r[7] = cd.flip;
        }
    }
    __syncthreads();
    SagittalRow row[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        row[s].ks0 = s_c[s].flip ? P2 - k1 : k0;
        row[s].in = (unsigned)j - (unsigned)s_c[s].lo[1] < (unsigned)s_c[s].n[1];
    }
    const float2 g = MIX ? s_g : make_float2(1.f, 0.f);

    // ---- images: stage (rows along W) ...
    const int rowf = TW * C, S = rowf | 1;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const PatchCand& cd = s_c[s];
        if (!row[s].in) continue;
        const unsigned u1 = (unsigned)j - (unsigned)cd.lo[1];
        for (int r = t; r < kTileH * rowf; r += 256) {
            const int kk = r / rowf, rem = r - kk * rowf, ii = rem / C, c = rem - ii * C;
            const unsigned u0 = (unsigned)(i0 + ii) - (unsigned)cd.lo[0], u2 = (unsigned)(row[s].ks0 + kk) - (unsigned)cd.lo[2];
            if (u0 < (unsigned)cd.n[0] && u2 < (unsigned)cd.n[2]) tile[s][kk * S + ii * C + c] = cd.img[box_voxel<kViewSagittal>(cd, u0, u1, u2) * C + c];
        }
    }
    __syncthreads();
    // ... and write (rows along k).  element (i0 + ii, j, ko, c) of sample s: staged inside its box, the fill outside
    auto image_at = [&](int s, int ii, int ko, int c) -> float {
        const PatchCand& cd = s_c[s];
        const int ks = cd.flip ? P2 - 1 - ko : ko;
        const unsigned u0 = (unsigned)(i0 + ii) - (unsigned)cd.lo[0], u2 = (unsigned)ks - (unsigned)cd.lo[2];
        if (row[s].in && u0 < (unsigned)cd.n[0] && u2 < (unsigned)cd.n[2]) return tile[s][(ks - row[s].ks0) * S + ii * C + c];
        return fill_value((((unsigned)(i0 + ii) * (unsigned)P1 + (unsigned)j) * (unsigned)P2 + (unsigned)ks) * (unsigned)C + (unsigned)c, cd.s_fill);
    };
    auto image_out = [&](int ii, int ko, int c) -> float {
        const float a = image_at(0, ii, ko, c);
        return MIX ? mix(g, a, image_at(NS - 1, ii, ko, c)) : a;
    };
    const int runf = kTileH * C, nkf = (k1 - k0) * C;  // floats of one i's run over (k, c): of a whole tile, of this one
    if (vec_i) {
        for (int r = t; r < TW * (runf / 4); r += 256) {
            const int ii = r / (runf / 4), q0 = (r - ii * (runf / 4)) * 4;
            if (i0 + ii >= P0 || q0 >= nkf) continue;  // nkf is a multiple of 4: a unit is inside or outside as a whole
            float v[4];
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                const int kk = (q0 + n) / C, c = (q0 + n) - kk * C;
                v[n] = image_out(ii, k0 + kk, c);
            }
            float* dst = out_i + ((((size_t)b * P0 + i0 + ii) * P1 + j) * P2 + k0) * C + q0;
            *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
        }
    } else {
        for (int r = t; r < TW * runf; r += 256) {
            const int ii = r / runf, q = r - ii * runf;
            if (i0 + ii >= P0 || q >= nkf) continue;
            const int kk = q / C, c = q - kk * C;
            out_i[((((size_t)b * P0 + i0 + ii) * P1 + j) * P2 + k0) * C + q] = image_out(ii, k0 + kk, c);
        }
    }
    __syncthreads();

    // ---- labels and weights through the same tile: label | weight << 8 per voxel, pitch TW | 1
    const int SV = TW | 1;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const PatchCand& cd = s_c[s];
        if (!row[s].in) continue;
        const unsigned u1 = (unsigned)j - (unsigned)cd.lo[1];
        unsigned* tv = reinterpret_cast<unsigned*>(tile[s]);
        for (int r = t; r < kTileH * TW; r += 256) {
            const int kk = r / TW, ii = r - kk * TW;
            const unsigned u0 = (unsigned)(i0 + ii) - (unsigned)cd.lo[0], u2 = (unsigned)(row[s].ks0 + kk) - (unsigned)cd.lo[2];
            if (u0 < (unsigned)cd.n[0] && u2 < (unsigned)cd.n[2]) {
                const size_t v = box_voxel<kViewSagittal>(cd, u0, u1, u2);
                tv[kk * SV + ii] = (unsigned)cd.lab[v] | (unsigned)cd.wgt[v] << 8;
            }
        }
    }
    __syncthreads();
    auto voxel_at = [&](int s, int ii, int ko) -> unsigned {  // 0 outside the copied box: label 0, weight 0
        const PatchCand& cd = s_c[s];
        const int ks = cd.flip ? P2 - 1 - ko : ko;
        const unsigned u0 = (unsigned)(i0 + ii) - (unsigned)cd.lo[0], u2 = (unsigned)ks - (unsigned)cd.lo[2];
        if (row[s].in && u0 < (unsigned)cd.n[0] && u2 < (unsigned)cd.n[2]) return reinterpret_cast<const unsigned*>(tile[s])[(ks - row[s].ks0) * SV + ii];
        return 0u;
    };
    auto weight_out = [&](int ii, int ko) -> float {  // the drawn sample's weight, or the or of the two
        unsigned w = voxel_at(0, ii, ko) >> 8;
        if (MIX) return (w | voxel_at(NS - 1, ii, ko) >> 8) != 0u ? 1.f : 0.f;
        return (float)w;
    };
    const int nk = k1 - k0;
    if (vec_v) {
        for (int r = t; r < TW * (kTileH / 4); r += 256) {
            const int ii = r / (kTileH / 4), q0 = (r - ii * (kTileH / 4)) * 4;
            if (i0 + ii >= P0 || q0 >= nk) continue;  // P2 % 4 == 0: a unit is inside or outside as a whole
            const size_t at = (((size_t)b * P0 + i0 + ii) * P1 + j) * P2 + k0 + q0;
            *reinterpret_cast<float4*>(out_w + at) =
                make_float4(weight_out(ii, k0 + q0), weight_out(ii, k0 + q0 + 1), weight_out(ii, k0 + q0 + 2), weight_out(ii, k0 + q0 + 3));
            if (!MIX)
                *reinterpret_cast<int4*>(out_l + at) = make_int4((int)(voxel_at(0, ii, k0 + q0) & 255u), (int)(voxel_at(0, ii, k0 + q0 + 1) & 255u),
                                                                 (int)(voxel_at(0, ii, k0 + q0 + 2) & 255u), (int)(voxel_at(0, ii, k0 + q0 + 3) & 255u));
        }
    } else {
        for (int r = t; r < TW * kTileH; r += 256) {
            const int ii = r / kTileH, kk = r - ii * kTileH;
            if (i0 + ii >= P0 || kk >= nk) continue;
            const size_t at = (((size_t)b * P0 + i0 + ii) * P1 + j) * P2 + k0 + kk;
            out_w[at] = weight_out(ii, k0 + kk);
            if (!MIX) out_l[at] = (int)(voxel_at(0, ii, k0 + kk) & 255u);
        }
    }
    if (MIX) {  // the soft rows, [.., k, K]: one run of nk * K floats per i
        const int runs = kTileH * K;
        for (int r = t; r < TW * runs; r += 256) {
            const int ii = r / runs, q = r - ii * runs, kk = q / K, cls = q - kk * K;
            if (i0 + ii >= P0 || kk >= nk) continue;
            const int l1 = (int)(voxel_at(0, ii, k0 + kk) & 255u), l2 = (int)(voxel_at(NS - 1, ii, k0 + kk) & 255u);
            out_s[((((size_t)b * P0 + i0 + ii) * P1 + j) * P2 + k0) * K + q] = mix_class(g, l1, l2, cls);
        }
    }
}

inline int volume_shape_ok(const char* who, int32_t C, int64_t D, int64_t H, int64_t W)
{
    PS_CHECK(C >= 1 && C <= PS_PATCH_MAX_C, "%s: C = %d, must be in [1, %d]", who, (int)C, PS_PATCH_MAX_C);
    PS_CHECK(D >= 1 && H >= 1 && W >= 1 && D < (1ll << 31) && H < (1ll << 31) && W < (1ll << 31) && D * H < (1ll << 31) && D * H * W < (1ll << 31),
             "%s: the volume is [%lld, %lld, %lld] (every extent >= 1, D * H * W < 2^31)", who, (long long)D, (long long)H, (long long)W);
    return PS_OK;
}

// what the two samplers check alike, in ps_patch_sample's order: `rows` rows of cand (the batch's slots, or the mixed batch's drawn samples)
inline int sampler_args_ok(const char* who, const float* const* images, const uint8_t* const* labels, const uint8_t* const* weights, const int64_t* dims,
                           int64_t n, int32_t C, const int32_t* cand, int rows, int32_t T, const int64_t* P, int32_t mode, bool outs, const char* out_names)
{
    PS_CHECK(T >= 1 && T <= PS_PATCH_MAX_T, "%s: T = %d, must be in [1, %d]", who, (int)T, PS_PATCH_MAX_T);
    PS_CHECK(mode == PS_PATCH_RANDOM || mode == PS_PATCH_ALL_POSITIVE || mode == PS_PATCH_ONE_POSITIVE, "%s: mode = %d is none of the three", who, (int)mode);
    PS_CHECK(n >= 1 && n < (1ll << 31), "%s: n = %lld volumes", who, (long long)n);
    PS_CHECK(images && labels && weights && dims && cand && P, "%s: NULL images, labels, weights, dims, cand or P table", who);
    PS_CHECK(outs, "%s: NULL %s", who, out_names);
    PS_CHECK(P[0] >= 1 && P[1] >= 1 && P[2] >= 1 && P[0] < (1ll << 31) && P[1] < (1ll << 31) && P[2] < (1ll << 31) && P[0] * P[1] < (1ll << 31)
                 && P[0] * P[1] * P[2] < (1ll << 31) && P[0] * P[1] * P[2] * C < (1ll << 31),
             "%s: P = [%lld, %lld, %lld] (every extent >= 1, P0 * P1 * P2 * C < 2^31)", who, (long long)P[0], (long long)P[1], (long long)P[2]);
    for (int64_t v = 0; v < n; ++v) {
        PS_CHECK(images[v] && labels[v] && weights[v], "%s: volume %lld has a NULL image, label or weight pointer", who, (long long)v);
        const int64_t* d = dims + 3 * v;
        PS_CHECK(d[0] >= 1 && d[1] >= 1 && d[2] >= 1 && d[0] < (1ll << 31) && d[1] < (1ll << 31) && d[2] < (1ll << 31) && d[0] * d[1] < (1ll << 31)
                     && d[0] * d[1] * d[2] < (1ll << 31) && d[0] * d[1] * d[2] * C < (1ll << 31),
                 "%s: dims of volume %lld are [%lld, %lld, %lld] (every dim >= 1, d * h * w * C < 2^31)", who, (long long)v, (long long)d[0], (long long)d[1],
                 (long long)d[2]);
    }
    for (int i = 0; i < rows * T; ++i)
        PS_CHECK(cand[i] >= 0 && cand[i] < n, "%s: cand[%d, %d] = %d is not a volume of the bank (%lld volumes)", who, i / T, i % T, (int)cand[i], (long long)n);
    return PS_OK;
}

// The host's blob, uploaded in one copy: [the table: every candidate's window][win: the windows the mode can ask for][their counts, zero]
// [extra bytes of the caller's].  forced: the row all of whose tries PS_PATCH_ONE_POSITIVE may ask for.
struct SamplerBlob {
    std::vector<char> host;
    size_t win_off, counts_off, extra_off;
    int windows;
};

// view: the PS_VIEW_* value P is given in; flip: one 0 / 1 per row, or NULL
inline void sampler_table(SamplerBlob& bl, const float* const* images, const uint8_t* const* labels, const uint8_t* const* weights, const int64_t* dims,
                          const int32_t* cand, int rows, int T, const int64_t* P, uint32_t seed, int mode, int forced, size_t extra_bytes, int view,
                          const int32_t* flip)
{
    const int nc = rows * T;
    std::vector<int> win;
    bl.win_off = pad256(sizeof(PatchCand) * nc);
    bl.counts_off = bl.win_off + pad256(sizeof(int) * nc);
    bl.extra_off = bl.counts_off + pad256(sizeof(unsigned) * nc);
    bl.host.assign(bl.extra_off + pad256(extra_bytes), 0);
    PatchCand* hc = reinterpret_cast<PatchCand*>(bl.host.data());
    for (int b = 0; b < rows; ++b)
        for (int t = 0; t < T; ++t) {
            PatchCand& cd = hc[b * T + t];
            const int v = cand[b * T + t];
            const unsigned s = hash32(seed + kSeedMul * (unsigned)(b * T + t + 1));
            cd.img = images[v], cd.lab = labels[v], cd.wgt = weights[v];
            const unsigned h[3] = {hash32(s + kAxisMul * 1u), hash32(s + kAxisMul * 2u), hash32(s + kAxisMul * 3u)};
            SamplerBox bx;
            sampler_box(view, dims + 3 * v, P, h, bx);
            for (int a = 0; a < 3; ++a) {
                cd.dim[a] = (int)dims[3 * v + a], cd.src[a] = bx.vsrc[a], cd.vn[a] = bx.vn[a];
                cd.c[a] = bx.c[a], cd.lo[a] = bx.lo[a], cd.n[a] = bx.n[a];
            }
            cd.s_fill = hash32(s + kAxisMul * 4u);
            cd.vol = v;
            cd.flip = flip ? flip[b] : 0;
            const bool counted = t == 0 || mode == PS_PATCH_ALL_POSITIVE || (mode == PS_PATCH_ONE_POSITIVE && b == forced);
            cd.count = counted ? (int)win.size() : -1;
            if (counted) win.push_back(b * T + t);
        }
    std::copy(win.begin(), win.end(), reinterpret_cast<int*>(bl.host.data() + bl.win_off));  // (the counts behind them stay zero)
    bl.windows = (int)win.size();
}

// the blob into the context's arena, and launch 1 over its windows; d_tab: where it lies on the device.  P: the patch as the VOLUME's
// axes see it (sampler_patch_in_volume)
inline int sampler_count(ps_context* c, const SamplerBlob& bl, const int64_t* P, char*& d_tab)
{
    hipStream_t st = c->stream;
    Arena& A = c->sample_arena;
    for (int pass = 0; pass < 2; ++pass) {
        A.begin(pass == 0);
        d_tab = A.take<char>(bl.host.size());
        if (pass == 0) PS_TRY(A.buf.reserve(A.off));
    }
    const unsigned kdw = (unsigned)((P[2] + 6) / 4);  // a row of P2 bytes starting at byte 3 of a word touches this many
    const unsigned count_blocks = (unsigned)(((size_t)P[0] * P[1] * kdw + 2047) / 2048);
    PS_TRY(c->upload_async(d_tab, bl.host.data(), bl.host.size()));
    hipLaunchKernelGGL(patch_count_kernel, dim3(count_blocks, (unsigned)bl.windows), dim3(256), 0, st, reinterpret_cast<const PatchCand*>(d_tab),
                       reinterpret_cast<const int*>(d_tab + bl.win_off), reinterpret_cast<unsigned*>(d_tab + bl.counts_off), kdw);
    return PS_OK;
}

}  // namespace

}  // namespace ps

using namespace ps;

extern "C" int ps_saliency_brats_measure(ps_context* c, const float* raw, int32_t C, int64_t D, int64_t H, int64_t W, int32_t margin, int64_t* box,
                                         double* stats)
{
    const char* who = "ps_saliency_brats_measure";
    PS_TRY(volume_shape_ok(who, C, D, H, W));
    PS_CHECK(margin >= 0, "%s: margin = %d is negative", who, (int)margin);
    PS_CHECK(raw && box && stats, "%s: NULL raw, box or stats", who);
    PS_CHECK(c, "%s: NULL context", who);
    PS_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const size_t nvox = (size_t)D * H * W;
    const int slabs = ceil_div((int64_t)nvox, kCropSlab);
    Arena& A = c->sample_arena;
    double *part = nullptr, *res = nullptr;
    for (int pass = 0; pass < 2; ++pass) {
        A.begin(pass == 0);
        part = A.take<double>((size_t)slabs * C * 2);
        res = A.take<double>(3 * (size_t)C + 3);  // [tot: C x (sum, count)][dev2: C][the raw min / max: 6 int]
        if (pass == 0) PS_TRY(A.buf.reserve(A.off));
    }
    double *tot = res, *dev2 = res + 2 * C;
    int* mm = reinterpret_cast<int*>(res + 3 * C);
    const int mm0[6] = {INT_MAX, INT_MAX, INT_MAX, -1, -1, -1};
    std::vector<char> h((3 * (size_t)C + 3) * sizeof(double));
    {
        Stage stg(c, "saliency_prepare", 5);
        PS_TRY(c->upload_async(mm, mm0, sizeof mm0));
        hipLaunchKernelGGL(brats_box_kernel, dim3((unsigned)std::min<size_t>(blocks256(nvox), 2048)), dim3(256), 0, st, raw, (unsigned)nvox, (int)H, (int)W, mm);
        const dim3 grid((unsigned)slabs, (unsigned)C);
        hipLaunchKernelGGL(brats_stats_kernel<false>, grid, dim3(256), 0, st, raw, nvox, (int)D, (int)H, (int)W, (int)margin, mm, tot, part);
        hipLaunchKernelGGL(reduce_partials_kernel<double>, dim3((unsigned)ceil_div(2 * C, 16)), dim3(256), 0, st, part, slabs, 2 * C, tot);
        hipLaunchKernelGGL(brats_stats_kernel<true>, grid, dim3(256), 0, st, raw, nvox, (int)D, (int)H, (int)W, (int)margin, mm, tot, part);
        hipLaunchKernelGGL(reduce_partials_kernel<double>, dim3((unsigned)ceil_div(C, 16)), dim3(256), 0, st, part, slabs, (int)C, dev2);
        PS_HIP(hipGetLastError());
        PS_HIP(hipMemcpyAsync(h.data(), res, h.size(), hipMemcpyDeviceToHost, st));
        PS_HIP(hipStreamSynchronize(st));
    }
    const double* ht = reinterpret_cast<const double*>(h.data());
    const int* hm = reinterpret_cast<const int*>(ht + 3 * C);
    PS_CHECK(hm[3] >= hm[0], "%s: raw[0] is all zero, there is no region to crop", who);
    const int64_t dims[3] = {D, H, W};
    int64_t b[6];
    for (int a = 0; a < 3; ++a) {
        b[a] = std::max<int64_t>(hm[a] - margin, 0);
        b[3 + a] = std::min<int64_t>((int64_t)hm[3 + a] + margin, dims[a] - 1);
    }
    std::vector<double> s(2 * (size_t)C);
    for (int m = 0; m < C; ++m) {
        const double n = ht[2 * m + 1];
        PS_CHECK(n > 0.0, "%s: modality %d has no voxel above zero inside the box (mean / std undefined)", who, m);
        s[2 * m] = ht[2 * m] / n;
        s[2 * m + 1] = std::sqrt(ht[2 * C + m] / n);
        PS_CHECK(s[2 * m + 1] > 0.0 && std::isfinite(s[2 * m + 1]) && std::isfinite(s[2 * m]),
                 "%s: modality %d has mean %g and std %g over its voxels above zero: it cannot be normalised", who, m, s[2 * m], s[2 * m + 1]);
    }
    std::copy(b, b + 6, box);
    std::copy(s.begin(), s.end(), stats);
    return PS_OK;
}

extern "C" int ps_saliency_brats_apply(ps_context* c, const float* raw, const int32_t* seg, int32_t C, int64_t D, int64_t H, int64_t W, int32_t num_class,
                                       const int64_t* box, const double* stats, float* image, uint8_t* label, uint8_t* weight)
{
    const char* who = "ps_saliency_brats_apply";
    PS_TRY(volume_shape_ok(who, C, D, H, W));
    PS_CHECK(num_class >= 2, "%s: num_class = %d, must be at least 2", who, (int)num_class);
    PS_CHECK(raw && box && stats && image && label && weight, "%s: NULL raw, box, stats, image, label or weight", who);
    const int64_t dims[3] = {D, H, W};
    ApplyArgs a;
    for (int k = 0; k < 3; ++k) {
        PS_CHECK(box[k] >= 0 && box[3 + k] >= box[k] && box[3 + k] < dims[k], "%s: box axis %d is [%lld, %lld] in a volume of %lld", who, k,
                 (long long)box[k], (long long)box[3 + k], (long long)dims[k]);
        a.box.lo[k] = (int)box[k];
        a.box.ext[k] = (int)(box[3 + k] - box[k] + 1);
    }
    for (int m = 0; m < C; ++m) {
        PS_CHECK(std::isfinite(stats[2 * m]) && std::isfinite(stats[2 * m + 1]) && stats[2 * m + 1] > 0.0, "%s: stats of modality %d are mean %g, std %g", who,
                 m, stats[2 * m], stats[2 * m + 1]);
        a.mean[m] = stats[2 * m];
        a.sd[m] = stats[2 * m + 1];
    }
    PS_CHECK(c, "%s: NULL context", who);
    PS_HIP(hipSetDevice(c->device));
    const unsigned ncrop = (unsigned)((size_t)a.box.ext[0] * a.box.ext[1] * a.box.ext[2]);
    Stage stg(c, "saliency_prepare", 1);
    hipLaunchKernelGGL(brats_apply_kernel, dim3(blocks256(ncrop)), dim3(256), 0, c->stream, raw, seg, (size_t)D * H * W, (int)H, (int)W, (int)C, (int)num_class,
                       a, ncrop, image, label, weight);
    PS_HIP(hipGetLastError());
    return PS_OK;
}

extern "C" int ps_saliency_pancreas_prepare(ps_context* c, const void* ct, int32_t dtype, int64_t n, const uint8_t* label, float* image, uint8_t* out_label,
                                            uint8_t* weight)
{
    const char* who = "ps_saliency_pancreas_prepare";
    PS_CHECK(dtype == PS_VOLUME_I16 || dtype == PS_VOLUME_F32, "%s: dtype = %d, must be PS_VOLUME_I16 or PS_VOLUME_F32", who, (int)dtype);
    PS_CHECK(n >= 1 && n < (1ll << 31), "%s: n = %lld voxels, must be in [1, 2^31)", who, (long long)n);
    PS_CHECK(ct && image && out_label && weight, "%s: NULL ct, image, out_label or weight", who);
    PS_CHECK(c, "%s: NULL context", who);
    PS_HIP(hipSetDevice(c->device));
    const dim3 grid((unsigned)std::min<size_t>(blocks256((size_t)n), 4096));
    Stage stg(c, "saliency_prepare", 1);
    if (dtype == PS_VOLUME_I16)
        hipLaunchKernelGGL(pancreas_prepare_kernel<int16_t>, grid, dim3(256), 0, c->stream, static_cast<const int16_t*>(ct), (size_t)n, label, image, out_label,
                           weight);
    else
        hipLaunchKernelGGL(pancreas_prepare_kernel<float>, grid, dim3(256), 0, c->stream, static_cast<const float*>(ct), (size_t)n, label, image, out_label, weight);
    PS_HIP(hipGetLastError());
    return PS_OK;
}


namespace ps {

namespace {

// what the view entries check on top of the old ones: the view, the flip bits (one per drawn sample), the sagittal gather's grid
inline int sampler_view_ok(const char* who, int32_t view, const int32_t* flip, int rows, int32_t B, int32_t C, const int64_t* P)
{
    PS_CHECK(view >= PS_VIEW_AXIAL && view <= PS_VIEW_CORONAL, "%s: view = %d, must be a PS_VIEW_* value (0, 1, 2)", who, (int)view);
    for (int i = 0; flip && i < rows; ++i) PS_CHECK(flip[i] == 0 || flip[i] == 1, "%s: flip[%d] = %d, must be 0 or 1", who, i, (int)flip[i]);
    if (view == PS_VIEW_SAGITTAL)
        PS_CHECK((int64_t)B * P[1] < (1ll << 24) && ceil_div(P[0], (int64_t)tile_w(C)) <= 65535 && ceil_div(P[2], (int64_t)kTileH) <= 65535,
                 "%s: the sagittal view takes B * P1 < 2^24, P0 <= 65535 * %d and P2 <= 65535 * %d, got B = %d, P = [%lld, %lld, %lld]", who, tile_w(C), kTileH,
                 (int)B, (long long)P[0], (long long)P[1], (long long)P[2]);
    return PS_OK;
}

template <int VIEW>
void gather_rows_launch(hipStream_t st, bool row4, unsigned blocks, const PatchCand* d_c, const unsigned* d_counts, const PatchShape& sh, unsigned img_blocks,
                        bool vec_i, bool vec_v, float* out_images, float* out_weights, int32_t* out_labels, int32_t* out_info)
{
    if (row4)
        hipLaunchKernelGGL((patch_gather_kernel<true, VIEW>), dim3(blocks), dim3(256), 0, st, d_c, d_counts, sh, img_blocks, vec_i, vec_v, out_images, out_weights,
                           out_labels, out_info);
    else
        hipLaunchKernelGGL((patch_gather_kernel<false, VIEW>), dim3(blocks), dim3(256), 0, st, d_c, d_counts, sh, img_blocks, vec_i, vec_v, out_images, out_weights,
                           out_labels, out_info);
}

template <int VIEW>
void mix_rows_launch(hipStream_t st, bool row4, unsigned blocks, const PatchCand* d_c, const unsigned* d_counts, const float2* d_g, const PatchShape& sh, int K,
                     unsigned img_blocks, bool vec_i, bool vec_w, int al_s, float* out_images, float* out_weights, float* out_soft, int32_t* out_info)
{
    if (row4)
        hipLaunchKernelGGL((patch_mix_kernel<true, VIEW>), dim3(blocks), dim3(256), 0, st, d_c, d_counts, d_g, sh, K, img_blocks, vec_i, vec_w, al_s, out_images,
                           out_weights, out_soft, out_info);
    else
        hipLaunchKernelGGL((patch_mix_kernel<false, VIEW>), dim3(blocks), dim3(256), 0, st, d_c, d_counts, d_g, sh, K, img_blocks, vec_i, vec_w, al_s, out_images,
                           out_weights, out_soft, out_info);
}

// the sagittal gather's grid: (slot, view row j) x tiles along i x tiles along k
inline dim3 sagittal_grid(int slots, const PatchShape& sh, int TW)
{
    return dim3((unsigned)(slots * sh.P[1]), (unsigned)ceil_div(sh.P[0], TW), (unsigned)ceil_div(sh.P[2], kTileH));
}

// the one body of ps_patch_sample (the axial view, no flip) and ps_patch_sample_view
int patch_sample(const char* who, ps_context* c, const float* const* images, const uint8_t* const* labels, const uint8_t* const* weights, const int64_t* dims,
                 int64_t n, int32_t C, const int32_t* cand, int32_t B, int32_t T, const int64_t* P, uint32_t seed, int32_t mode, int32_t view,
                 const int32_t* flip, float* out_images, float* out_weights, int32_t* out_labels, int32_t* out_info)
{
    // every argument error is found here, before anything is enqueued
    PS_CHECK(C >= 1 && C <= PS_PATCH_MAX_C, "%s: C = %d, must be in [1, %d]", who, (int)C, PS_PATCH_MAX_C);
    PS_CHECK(B >= 1 && B <= PS_PATCH_MAX_B, "%s: B = %d, must be in [1, %d]", who, (int)B, PS_PATCH_MAX_B);
    PS_TRY(sampler_args_ok(who, images, labels, weights, dims, n, C, cand, B, T, P, mode, out_images && out_weights && out_labels && out_info,
                           "out_images, out_weights, out_labels or out_info"));
    PS_TRY(sampler_view_ok(who, view, flip, B, B, C, P));
    PS_CHECK(c, "%s: NULL context", who);

    SamplerBlob bl;
    sampler_table(bl, images, labels, weights, dims, cand, B, T, P, seed, mode, B - 1, 0, view, flip);
    int64_t PV[3];
    sampler_patch_in_volume(view, P, PV);
    PS_HIP(hipSetDevice(c->device));
    PatchShape sh;
    sh.P[0] = (int)P[0], sh.P[1] = (int)P[1], sh.P[2] = (int)P[2], sh.C = C, sh.B = B, sh.T = T, sh.mode = mode;
    const size_t V = (size_t)P[0] * P[1] * P[2];
    const unsigned img_blocks = (unsigned)(((size_t)B * V * C + 4095) / 4096), vox_blocks = (unsigned)(((size_t)B * V + 4095) / 4096);
    const bool vec_i = (reinterpret_cast<uintptr_t>(out_images) & 15) == 0;
    const bool vec_v = ((reinterpret_cast<uintptr_t>(out_weights) | reinterpret_cast<uintptr_t>(out_labels)) & 15) == 0;
    Stage stg(c, "patch_sample", 2);
    char* d_tab = nullptr;
    PS_TRY(sampler_count(c, bl, PV, d_tab));
    const PatchCand* d_c = reinterpret_cast<const PatchCand*>(d_tab);
    const unsigned* d_counts = reinterpret_cast<const unsigned*>(d_tab + bl.counts_off);
    const bool row4 = (P[2] * C) % 4 == 0;
    if (view == PS_VIEW_AXIAL)
        gather_rows_launch<kViewAxial>(c->stream, row4, img_blocks + vox_blocks, d_c, d_counts, sh, img_blocks, vec_i, vec_v, out_images, out_weights, out_labels,
                                       out_info);
    else if (view == PS_VIEW_CORONAL)
        gather_rows_launch<kViewCoronal>(c->stream, row4, img_blocks + vox_blocks, d_c, d_counts, sh, img_blocks, vec_i, vec_v, out_images, out_weights, out_labels,
                                         out_info);
    else {
        const int TW = tile_w(C);
        hipLaunchKernelGGL(patch_gather_sagittal_kernel<false>, sagittal_grid(B, sh, TW), dim3(256), 0, c->stream, d_c, d_counts, (const float2*)nullptr, sh, 0, TW,
                           vec_i && row4, vec_v && P[2] % 4 == 0, out_images, out_weights, out_labels, (float*)nullptr, out_info);
    }
    PS_HIP(hipGetLastError());
    return PS_OK;
}

// the one body of ps_patch_sample_mixup (the axial view, no flip) and ps_patch_sample_mixup_view
int patch_sample_mixup(const char* who, ps_context* c, const float* const* images, const uint8_t* const* labels, const uint8_t* const* weights,
                       const int64_t* dims, int64_t n, int32_t C, const int32_t* cand, int32_t B, int32_t T, const int64_t* P, uint32_t seed, int32_t mode,
                       int32_t num_classes, const double* gamma, int32_t view, const int32_t* flip, float* out_images, float* out_weights, float* out_soft,
                       int32_t* out_info)
{
    // every argument error is found here, before anything is enqueued
    PS_CHECK(C >= 1 && C <= PS_PATCH_MAX_C, "%s: C = %d, must be in [1, %d]", who, (int)C, PS_PATCH_MAX_C);
    PS_CHECK(B >= 1 && B <= PS_PATCH_MAX_B - 1, "%s: B = %d, must be in [1, %d] (B + 1 samples are drawn)", who, (int)B, PS_PATCH_MAX_B - 1);
    PS_CHECK(num_classes >= 2 && num_classes <= 16, "%s: num_classes = %d, must be in [2, 16]", who, (int)num_classes);
    PS_TRY(sampler_args_ok(who, images, labels, weights, dims, n, C, cand, B + 1, T, P, mode, out_images && out_weights && out_soft && out_info,
                           "out_images, out_weights, out_soft or out_info"));
    PS_CHECK((int64_t)B * P[0] * P[1] * P[2] * num_classes < (1ll << 31), "%s: B * P0 * P1 * P2 * num_classes = %lld, must stay below 2^31", who,
             (long long)((int64_t)B * P[0] * P[1] * P[2] * num_classes));
    PS_CHECK(gamma, "%s: NULL gamma", who);
    for (int b = 0; b < B; ++b)
        PS_CHECK(std::isfinite(gamma[b]) && gamma[b] >= 0.0 && gamma[b] <= 1.0, "%s: gamma[%d] = %g, must be finite and in [0, 1]", who, b, gamma[b]);
    PS_TRY(sampler_view_ok(who, view, flip, B + 1, B, C, P));
    PS_CHECK(c, "%s: NULL context", who);

    SamplerBlob bl;
    sampler_table(bl, images, labels, weights, dims, cand, B + 1, T, P, seed, mode, B - 1, sizeof(float2) * B, view, flip);
    int64_t PV[3];
    sampler_patch_in_volume(view, P, PV);
    float* hg = reinterpret_cast<float*>(bl.host.data() + bl.extra_off);
    for (int b = 0; b < B; ++b) {
        hg[2 * b] = (float)gamma[b];
        hg[2 * b + 1] = (float)(1.0 - gamma[b]);  // (the subtraction in float64, as NumPy's scalar times a float32 array)
    }
    PS_HIP(hipSetDevice(c->device));
    PatchShape sh;
    sh.P[0] = (int)P[0], sh.P[1] = (int)P[1], sh.P[2] = (int)P[2], sh.C = C, sh.B = B, sh.T = T, sh.mode = mode;
    const size_t V = (size_t)P[0] * P[1] * P[2];
    const unsigned img_blocks = (unsigned)(((size_t)B * V * C + 4095) / 4096), vox_blocks = (unsigned)(((size_t)B * V + 4095) / 4096);
    const bool vec_i = (reinterpret_cast<uintptr_t>(out_images) & 15) == 0, vec_w = (reinterpret_cast<uintptr_t>(out_weights) & 15) == 0;
    const uintptr_t as = reinterpret_cast<uintptr_t>(out_soft);
    const int al_s = (as & 15) == 0 ? 16 : (as & 7) == 0 ? 8 : 4;
    Stage stg(c, "patch_sample_mixup", 2);
    char* d_tab = nullptr;
    PS_TRY(sampler_count(c, bl, PV, d_tab));
    const PatchCand* d_c = reinterpret_cast<const PatchCand*>(d_tab);
    const unsigned* d_counts = reinterpret_cast<const unsigned*>(d_tab + bl.counts_off);
    const float2* d_g = reinterpret_cast<const float2*>(d_tab + bl.extra_off);
    const bool row4 = (P[2] * C) % 4 == 0;
    if (view == PS_VIEW_AXIAL)
        mix_rows_launch<kViewAxial>(c->stream, row4, img_blocks + vox_blocks, d_c, d_counts, d_g, sh, (int)num_classes, img_blocks, vec_i, vec_w, al_s, out_images,
                                    out_weights, out_soft, out_info);
    else if (view == PS_VIEW_CORONAL)
        mix_rows_launch<kViewCoronal>(c->stream, row4, img_blocks + vox_blocks, d_c, d_counts, d_g, sh, (int)num_classes, img_blocks, vec_i, vec_w, al_s, out_images,
                                      out_weights, out_soft, out_info);
    else {
        const int TW = tile_w(C);
        hipLaunchKernelGGL(patch_gather_sagittal_kernel<true>, sagittal_grid(B, sh, TW), dim3(256), 0, c->stream, d_c, d_counts, d_g, sh, (int)num_classes, TW,
                           vec_i && row4, vec_w && P[2] % 4 == 0, out_images, out_weights, (int32_t*)nullptr, out_soft, out_info);
    }
    PS_HIP(hipGetLastError());
    return PS_OK;
}

}  // namespace

}  // namespace ps

extern "C" int ps_patch_sample(ps_context* c, const float* const* images, const uint8_t* const* labels, const uint8_t* const* weights, const int64_t* dims,
                               int64_t n, int32_t C, const int32_t* cand, int32_t B, int32_t T, const int64_t* P, uint32_t seed, int32_t mode,
                               float* out_images, float* out_weights, int32_t* out_labels, int32_t* out_info)
{
    return patch_sample("ps_patch_sample", c, images, labels, weights, dims, n, C, cand, B, T, P, seed, mode, PS_VIEW_AXIAL, nullptr, out_images, out_weights,
                        out_labels, out_info);
}

extern "C" int ps_patch_sample_view(ps_context* c, const float* const* images, const uint8_t* const* labels, const uint8_t* const* weights, const int64_t* dims,
                                    int64_t n, int32_t C, const int32_t* cand, int32_t B, int32_t T, const int64_t* P, uint32_t seed, int32_t mode, int32_t view,
                                    const int32_t* flip, float* out_images, float* out_weights, int32_t* out_labels, int32_t* out_info)
{
    return patch_sample("ps_patch_sample_view", c, images, labels, weights, dims, n, C, cand, B, T, P, seed, mode, view, flip, out_images, out_weights, out_labels,
                        out_info);
}

extern "C" int ps_patch_sample_mixup(ps_context* c, const float* const* images, const uint8_t* const* labels, const uint8_t* const* weights,
                                     const int64_t* dims, int64_t n, int32_t C, const int32_t* cand, int32_t B, int32_t T, const int64_t* P, uint32_t seed,
                                     int32_t mode, int32_t num_classes, const double* gamma, float* out_images, float* out_weights, float* out_soft,
                                     int32_t* out_info)
{
    return patch_sample_mixup("ps_patch_sample_mixup", c, images, labels, weights, dims, n, C, cand, B, T, P, seed, mode, num_classes, gamma, PS_VIEW_AXIAL,
                              nullptr, out_images, out_weights, out_soft, out_info);
}

extern "C" int ps_patch_sample_mixup_view(ps_context* c, const float* const* images, const uint8_t* const* labels, const uint8_t* const* weights,
                                          const int64_t* dims, int64_t n, int32_t C, const int32_t* cand, int32_t B, int32_t T, const int64_t* P, uint32_t seed,
                                          int32_t mode, int32_t num_classes, const double* gamma, int32_t view, const int32_t* flip, float* out_images,
                                          float* out_weights, float* out_soft, int32_t* out_info)
{
    return patch_sample_mixup("ps_patch_sample_mixup_view", c, images, labels, weights, dims, n, C, cand, B, T, P, seed, mode, num_classes, gamma, view, flip,
                              out_images, out_weights, out_soft, out_info);
}
