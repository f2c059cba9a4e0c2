// metrics.hip -- the evaluation side of the reference on the device: what turns logits and probability volumes into reported numbers.
//
//   ps_confusion_accumulate   Network.evaluate's argmax + sklearn confusion_matrix (PointSegment/RandLANet.py:208-264), including the
//                             ignored-label handling of :226-233 (through a label map, Trainer.label_map's convention: -1 = ignored).
//                             The prediction is the argmax of the LOGITS with ties to the lowest index (np.argmax); the reference takes
//                             the argmax of the softmax, which differs only where distinct logits round to equal fp32 probabilities.
//   ps_probs_to_labels        genSegmentation's argmax + label remap (utils/genSegmentationBraTS.py:67-79)
//   ps_seg_metrics            Dice of label sets (utils/evaluationBraTS.py:22-64, evaluationPancreas.py:14-37) and medpy's hd95 with
//                             connectivity 1 (the scipy parts imported at evaluationBraTS.py:13-21)
//
// HD95 route: medpy's own.  For a mask pair (P, T): border(M) = M ^ erode(M) with the 6-neighbourhood and a zero outside the array;
// d_PT = EDT(~border(T)) sampled at border(P), d_TP the other way round; hd95 = np.percentile(hstack(d_PT, d_TP), 95) (linear rule).
// The EDT is separable: three passes, one per axis, each an exact 1-D min-plus transform f'(x) = min_q f(q) + (w (x - q))^2 over the
// line, in float64 (exact integers at unit spacing).  Each workgroup holds G lines in LDS and keeps only the finite entries of a line as
// candidates, so the first pass (from the border flags) and the second (only lines that met a border) cost what the border costs; the
// last pass evaluates only the voxels whose distance is read.  The two order statistics of the 95th percentile are picked by an eight-round
// MSB-first radix select over the float64 bit patterns of the squared distances (non-negative: they order as unsigned integers), with
// integer histograms -- nothing is sorted, nothing but the R x 5 results leaves the device, and every step is exact or a min, so the results
// are bitwise reproducible.  (The kd-tree route -- compaction, a tree per side, K = 1 searches -- needs the border counts on the host
// before it can plan its trees: a second synchronisation per call.  DESIGN.md "N5" has the measured times.)
#include "common.h"

#include <cmath>

namespace ps {

constexpr int kMetricClasses = 32;   // C of ps_confusion_accumulate / ps_probs_to_labels
constexpr int kMetricRegions = 8;    // R of ps_seg_metrics (2R border bits per voxel in a u16)
constexpr int kEdtLineElems = 6144;  // G * L of one EDT workgroup: G*L*24 (+8) bytes of LDS <= 144 KB
constexpr int kEdtMaxLines = 8;

// ------------------------------------------------------------------------------------------------------------------------------------
// confusion matrix
// ------------------------------------------------------------------------------------------------------------------------------------
// np.argmax: the first maximum; a NaN counts as the maximum (its first occurrence wins)
__device__ __forceinline__ bool argmax_takes(float v, float best) { return v > best || (v != v && best == best); }

__global__ __launch_bounds__(256) void confusion_kernel(const float* __restrict__ logits, const int32_t* __restrict__ labels, int64_t n, int C,
                                                        const int32_t* __restrict__ map, int L, unsigned long long* __restrict__ cm)
{
    __shared__ unsigned hist[kMetricClasses * kMetricClasses];
    for (int i = threadIdx.x; i < C * C; i += 256) hist[i] = 0;
    __syncthreads();
    for (int64_t row = blockIdx.x * (int64_t)256 + threadIdx.x; row < n; row += (int64_t)gridDim.x * 256) {
        int t = labels[row];
        if (map) t = (t >= 0 && t < L) ? map[t] : -1;
        if (t < 0 || t >= C) continue;  // ignored (or out of range: never counted)
        const float* r = logits + row * C;
        float best = r[0];
        int arg = 0;
        for (int c = 1; c < C; ++c) {
            const float v = r[c];
            if (argmax_takes(v, best)) { best = v; arg = c; }
        }
        atomicAdd(&hist[t * C + arg], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < C * C; i += 256)
        if (hist[i]) atomicAdd(&cm[i], (unsigned long long)hist[i]);
}

// ------------------------------------------------------------------------------------------------------------------------------------
// probability volume -> label volume
// ------------------------------------------------------------------------------------------------------------------------------------
struct LabelLut {
    uint8_t v[kMetricClasses];
};

__global__ __launch_bounds__(256) void probs_to_labels4_kernel(const float4* __restrict__ probs, int64_t V, LabelLut lut, uint8_t* __restrict__ out)
{
    __shared__ uint8_t s_lut[4];
    if (threadIdx.x < 4) s_lut[threadIdx.x] = lut.v[threadIdx.x];
    __syncthreads();
    for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < V; i += (int64_t)gridDim.x * 256) {
        const float4 p = probs[i];  // one voxel = 16 bytes per lane
        float best = p.x;
        int arg = 0;
        if (argmax_takes(p.y, best)) { best = p.y; arg = 1; }
        if (argmax_takes(p.z, best)) { best = p.z; arg = 2; }
        if (argmax_takes(p.w, best)) { best = p.w; arg = 3; }
        out[i] = s_lut[arg];
    }
}

__global__ __launch_bounds__(256) void probs_to_labels_kernel(const float* __restrict__ probs, int64_t V, int C, LabelLut lut, uint8_t* __restrict__ out)
{
    __shared__ uint8_t s_lut[kMetricClasses];
    if (threadIdx.x < kMetricClasses) s_lut[threadIdx.x] = lut.v[threadIdx.x];
    __syncthreads();
    for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < V; i += (int64_t)gridDim.x * 256) {
        const float* r = probs + i * C;
        float best = r[0];
        int arg = 0;
        for (int c = 1; c < C; ++c) {
            const float v = r[c];
            if (argmax_takes(v, best)) { best = v; arg = c; }
        }
        out[i] = s_lut[arg];
    }
}

// ------------------------------------------------------------------------------------------------------------------------------------
// region metrics
// ------------------------------------------------------------------------------------------------------------------------------------
struct SegState {
    unsigned long long cnt[kMetricRegions][5];     // n_pred, n_truth, n_both, border(P), border(T)
    unsigned long long rank[kMetricRegions][2];    // remaining rank of the lower / upper order statistic inside the current prefix
    unsigned long long prefix[kMetricRegions][2];  // bits of the order statistic found so far
    int active[kMetricRegions];                    // both borders non-empty: the selection runs
    unsigned hist[kMetricRegions][2][256];         // (zero between rounds)
    long long out_counts[kMetricRegions][3];       // the results: the only bytes the host reads
    double out_scores[kMetricRegions][2];
};

struct SegGeom {
    int d[3];
    int s[3];  // element strides (V < 2^31: 32-bit index arithmetic throughout)
    int V;
};

struct RegionTable {
    unsigned m[kMetricRegions];  // bit L = label L belongs to the region
};

__device__ __forceinline__ bool in_region(unsigned mask, unsigned label) { return label < 32 && ((mask >> label) & 1u); }

// counts and border flags of every region, one pass: bit 2r of flags[v] = v is on the border of pred's region r, bit 2r+1 = truth's
__global__ __launch_bounds__(256) void seg_mask_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ truth, SegGeom g, int R,
                                                       RegionTable reg, uint16_t* __restrict__ flags, SegState* __restrict__ st)
{
    __shared__ unsigned s_cnt[kMetricRegions * 5];
    if (threadIdx.x < R * 5) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    // every lane of a wave runs the same trip count (ballots below): lanes past the end carry "outside every mask"
    const unsigned stride = gridDim.x * 256u;
    const unsigned n_iter = ((unsigned)g.V + stride - 1) / stride;
    for (unsigned it = 0; it < n_iter; ++it) {
        const unsigned v = it * stride + blockIdx.x * 256u + threadIdx.x;
        const bool valid = v < (unsigned)g.V;
        unsigned lp[7] = {255, 255, 255, 255, 255, 255, 255}, lt[7] = {255, 255, 255, 255, 255, 255, 255};  // self + 6 neighbours (255: outside)
        if (valid) {
            const unsigned i2 = v % (unsigned)g.d[2], i1 = (v / (unsigned)g.d[2]) % (unsigned)g.d[1], i0 = v / (unsigned)g.s[0];
            const unsigned ii[3] = {i0, i1, i2};
            lp[0] = pred[v];
            lt[0] = truth[v];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                if (ii[a] > 0) { lp[1 + 2 * a] = pred[v - g.s[a]]; lt[1 + 2 * a] = truth[v - g.s[a]]; }
                if (ii[a] + 1 < (unsigned)g.d[a]) { lp[2 + 2 * a] = pred[v + g.s[a]]; lt[2 + 2 * a] = truth[v + g.s[a]]; }
            }
        }
        unsigned fl = 0;
        for (int r = 0; r < R; ++r) {
            const unsigned m = reg.m[r];
            const bool p = in_region(m, lp[0]), t = in_region(m, lt[0]);
            bool bp = false, bt = false;
#pragma unroll
            for (int k = 1; k < 7; ++k) {
                bp |= !in_region(m, lp[k]);
                bt |= !in_region(m, lt[k]);
            }
            bp &= p;
            bt &= t;
            fl |= (unsigned)bp << (2 * r) | (unsigned)bt << (2 * r + 1);
            const bool c[5] = {p, t, p && t, bp, bt};
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                const unsigned long long b = __ballot(c[k]);
                if (lane == 0 && b) atomicAdd(&s_cnt[r * 5 + k], (unsigned)__popcll(b));
            }
        }
        if (valid) flags[v] = (uint16_t)fl;
    }
    __syncthreads();
    if (threadIdx.x < R * 5 && s_cnt[threadIdx.x]) atomicAdd(&st->cnt[threadIdx.x / 5][threadIdx.x % 5], (unsigned long long)s_cnt[threadIdx.x]);
}

// One pass of the separable EDT along axis `a` over the 2R volumes (blockIdx.y = volume k: region k/2; k even = distance to truth's border,
// read at pred's border voxels; k odd = the other way round -- so volume k is read where flag bit k is set).
// FIRST: the input is the border flags (0 on the border of the other side, +inf elsewhere).  LAST: only voxels with flag bit k are computed.
// Lines of axis a are enumerated with the fastest-varying other axis first, so the G lines of a workgroup are neighbours in memory.
template <bool FIRST, bool LAST>
__global__ __launch_bounds__(256) void edt_pass_kernel(double* __restrict__ edt, const uint16_t* __restrict__ flags, SegGeom g, int a, int b, int c,
                                                       int G, double w)
{
    extern __shared__ double lds[];
    const int L = g.d[a];
    double* f = lds;                                                // [G][L] input, then output
    double2* cand = reinterpret_cast<double2*>(lds + (((size_t)G * L + 1) & ~(size_t)1));  // [G][L] (q * w, f(q)) of the finite entries, ascending q
    __shared__ int s_cnt[kEdtMaxLines];
    const int k = blockIdx.y;
    double* vol = edt + (size_t)k * (unsigned)g.V;
    const unsigned src_bit = (k & 1) ? (unsigned)(k - 1) : (unsigned)(k + 1);  // the border the distance is measured to
    const int nb = g.d[b];
    const int lines = nb * g.d[c];
    const int line0 = blockIdx.x * G;
    const int gl = min(G, lines - line0);
    const int tot = gl * L;
    auto voxel = [&](int ln, int x) -> int {
        const int j = line0 + ln;
        return (j % nb) * g.s[b] + (j / nb) * g.s[c] + x * g.s[a];
    };
    // global <-> LDS: along the contiguous axis walk x first; across it walk the gl neighbouring lines first (coalesced either way)
    const bool xfast = a == 2;
    auto split = [&](int idx, int& ln, int& x) {
        if (xfast) { ln = idx / L; x = idx - ln * L; }
        else { x = idx / gl; ln = idx - x * gl; }
    };
    for (int idx = threadIdx.x; idx < tot; idx += 256) {
        int ln, x;
        split(idx, ln, x);
        const int o = voxel(ln, x);
        double v;
        if (FIRST) v = ((flags[o] >> src_bit) & 1u) ? 0.0 : INFINITY;
        else v = vol[o];
        f[ln * L + x] = v;
    }
    __syncthreads();
    // compaction of the finite entries, one wave per line, ascending q (a min does not depend on the order; this keeps the loop uniform)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int ln = wave; ln < gl; ln += 4) {
        int n = 0;
        for (int x0 = 0; x0 < L; x0 += 64) {
            const int x = x0 + lane;
            const double v = x < L ? f[ln * L + x] : INFINITY;
            const bool fin = v < INFINITY;
            const unsigned long long m = __ballot(fin);
            if (fin) cand[ln * L + n + __popcll(m & ((1ull << lane) - 1))] = make_double2((double)x * w, v);
            n += __popcll(m);
        }
        if (lane == 0) s_cnt[ln] = n;
    }
    __syncthreads();
    // the transform: lanes of a wave on one line (x fastest), so the candidate reads are LDS broadcasts
    for (int idx = threadIdx.x; idx < tot; idx += 256) {
        const int ln = idx / L, x = idx - ln * L;
        if (LAST && !((flags[voxel(ln, x)] >> k) & 1u)) continue;
        const double xw = (double)x * w;
        const double2* cl = cand + ln * L;
        const int n = s_cnt[ln];
        double best = INFINITY;
        int j = 0;
        for (; j + 4 <= n; j += 4) {
            const double2 c0 = cl[j], c1 = cl[j + 1], c2 = cl[j + 2], c3 = cl[j + 3];
            const double d0 = xw - c0.x, d1 = xw - c1.x, d2 = xw - c2.x, d3 = xw - c3.x;
            best = fmin(best, fmin(fmin(d0 * d0 + c0.y, d1 * d1 + c1.y), fmin(d2 * d2 + c2.y, d3 * d3 + c3.y)));
        }
        for (; j < n; ++j) {
            const double d = xw - cl[j].x;
            best = fmin(best, d * d + cl[j].y);
        }
        f[ln * L + x] = best;  // (every candidate was copied into `cand`: f is free)
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < tot; idx += 256) {
        int ln, x;
        split(idx, ln, x);
        const int o = voxel(ln, x);
        if (LAST && !((flags[o] >> k) & 1u)) continue;  // (only these are read by the selection)
        vol[o] = f[ln * L + x];
    }
}

// ranks of numpy's linear percentile: virtual index (n - 1) * 0.95, the order statistics at floor() and floor() + 1 (clipped to n - 1)
__global__ void seg_rank_kernel(SegState* __restrict__ st, int R)
{
    const int r = threadIdx.x;
    if (r >= R) return;
    const unsigned long long nbp = st->cnt[r][3], nbt = st->cnt[r][4];
    st->active[r] = nbp > 0 && nbt > 0;
    const unsigned long long n = nbp + nbt;
    if (!n) return;
    const double vi = (double)(n - 1) * 0.95;
    unsigned long long lo = (unsigned long long)floor(vi);
    if (vi >= (double)(n - 1)) lo = n - 1;
    st->rank[r][0] = lo;
    st->rank[r][1] = lo + 1 < n ? lo + 1 : n - 1;
}

// one radix-select round: histogram of the 8-bit digit at `shift` of the keys that match the prefix so far
__global__ __launch_bounds__(256) void seg_select_hist_kernel(const double* __restrict__ edt, const uint16_t* __restrict__ flags, int V, int R,
                                                              int shift, SegState* __restrict__ st)
{
    __shared__ unsigned h[kMetricRegions * 2 * 256];
    __shared__ unsigned long long s_pre[kMetricRegions][2];
    __shared__ int s_act[kMetricRegions];
    for (int i = threadIdx.x; i < R * 512; i += 256) h[i] = 0;
    if (threadIdx.x < R * 2) s_pre[threadIdx.x >> 1][threadIdx.x & 1] = st->prefix[threadIdx.x >> 1][threadIdx.x & 1];
    if (threadIdx.x < R) s_act[threadIdx.x] = st->active[threadIdx.x];
    __syncthreads();
    const unsigned long long hi_mask = shift >= 56 ? 0ull : ~0ull << (shift + 8);
    for (int v = blockIdx.x * 256 + threadIdx.x; v < V; v += gridDim.x * 256) {
        const unsigned fl = flags[v];
        if (!fl) continue;
        for (int r = 0; r < R; ++r) {
            if (!s_act[r]) continue;
            for (int s = 0; s < 2; ++s) {
                const int k = 2 * r + s;
                if (!((fl >> k) & 1u)) continue;
                const unsigned long long key = (unsigned long long)__double_as_longlong(edt[(size_t)k * (unsigned)V + v]);
                const unsigned dig = (unsigned)(key >> shift) & 255u;
                for (int j = 0; j < 2; ++j)
                    if (((key ^ s_pre[r][j]) & hi_mask) == 0) atomicAdd(&h[(r * 2 + j) * 256 + dig], 1u);
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < R * 512; i += 256)
        if (h[i]) atomicAdd(&st->hist[i >> 9][(i >> 8) & 1][i & 255], h[i]);
}

// the digit whose bucket holds the remaining rank; clears the histogram for the next round
__global__ void seg_select_pick_kernel(SegState* __restrict__ st, int R, int shift)
{
    const int t = threadIdx.x;
    if (t >= 2 * R) return;
    const int r = t >> 1, j = t & 1;
    unsigned* h = st->hist[r][j];
    if (st->active[r]) {
        unsigned long long k = st->rank[r][j], below = 0;
        int d = 0;
        for (; d < 255; ++d) {
            if (k < below + h[d]) break;
            below += h[d];
        }
        st->rank[r][j] = k - below;
        st->prefix[r][j] |= (unsigned long long)d << shift;
    }
    for (int d = 0; d < 256; ++d) h[d] = 0;
}

__global__ void seg_finish_kernel(SegState* __restrict__ st, int R)
{
    const int r = threadIdx.x;
    if (r >= R) return;
    const unsigned long long np = st->cnt[r][0], nt = st->cnt[r][1], nb = st->cnt[r][2];
    st->out_counts[r][0] = (long long)np;
    st->out_counts[r][1] = (long long)nt;
    st->out_counts[r][2] = (long long)nb;
    // evaluationBraTS.py:22-25
    st->out_scores[r][0] = (np + nt) == 0 ? 1.0 : 2.0 * (double)nb / (double)(np + nt);
    double hd;
    if (np == 0 && nt == 0) hd = 0.0;
    else if (np == 0 || nt == 0) hd = INFINITY;
    else {
        const unsigned long long n = st->cnt[r][3] + st->cnt[r][4];
        const double vi = (double)(n - 1) * 0.95;
        const double gamma = vi - floor(vi);  // numpy: virtual - previous
        const double a = sqrt(__longlong_as_double((long long)st->prefix[r][0])), b = sqrt(__longlong_as_double((long long)st->prefix[r][1]));
        const double diff = b - a;
        // numpy's _lerp: a + (b - a) t, or b - (b - a)(1 - t) where t >= 0.5
        hd = gamma >= 0.5 ? b - diff * (1.0 - gamma) : a + diff * gamma;
        if (vi >= (double)(n - 1)) hd = b;  // (a single value: lo == hi)
    }
    st->out_scores[r][1] = hd;
}

static size_t al256(size_t b) { return (b + 255) & ~size_t(255); }

static size_t seg_scratch_bytes(int64_t V, int R) { return al256(sizeof(SegState)) + al256((size_t)V * 2) + (size_t)2 * R * V * sizeof(double); }

}  // namespace ps

using namespace ps;

extern "C" int ps_confusion_accumulate(ps_context* c, const float* logits, const int32_t* labels, int64_t n, int64_t C, const int32_t* label_map,
                                       int64_t L, int64_t* confusion)
{
    PS_CHECK(c && confusion, "ps_confusion_accumulate: NULL argument");
    PS_CHECK(C >= 1 && C <= kMetricClasses, "ps_confusion_accumulate: num_classes must be in [1, %d] (got %lld)", kMetricClasses, (long long)C);
    PS_CHECK(n >= 0, "ps_confusion_accumulate: negative n");
    PS_CHECK(n == 0 || (logits && labels), "ps_confusion_accumulate: logits / labels are NULL");
    PS_CHECK(!label_map || (L >= 1 && L < (1ll << 31)), "ps_confusion_accumulate: label_map needs 1 <= L < 2^31 entries");
    if (n == 0) return PS_OK;
    PS_HIP(hipSetDevice(c->device));
    Stage stg(c, "confusion", 1);
    const int grid = std::min(ceil_div(n, 256), 1024);
    hipLaunchKernelGGL(confusion_kernel, dim3(grid), dim3(256), 0, c->stream, logits, labels, n, (int)C, label_map, (int)(label_map ? L : 0),
                       reinterpret_cast<unsigned long long*>(confusion));
    PS_HIP(hipGetLastError());
    return PS_OK;
}

extern "C" int ps_probs_to_labels(ps_context* c, const float* probs, int64_t V, int64_t C, const int32_t* label_values, uint8_t* labels)
{
    PS_CHECK(c && label_values, "ps_probs_to_labels: NULL argument");
    PS_CHECK(C >= 1 && C <= kMetricClasses, "ps_probs_to_labels: C must be in [1, %d] (got %lld)", kMetricClasses, (long long)C);
    PS_CHECK(V >= 0, "ps_probs_to_labels: negative V");
    PS_CHECK(V == 0 || (probs && labels), "ps_probs_to_labels: probs / labels are NULL");
    LabelLut lut = {};
    for (int i = 0; i < C; ++i) {
        PS_CHECK(label_values[i] >= 0 && label_values[i] <= 255, "ps_probs_to_labels: label_values[%d] = %d does not fit uint8", i, label_values[i]);
        lut.v[i] = (uint8_t)label_values[i];
    }
    if (V == 0) return PS_OK;
    PS_HIP(hipSetDevice(c->device));
    Stage stg(c, "probs_to_labels", 1);
    const int grid = std::min(ceil_div(V, 256), 2048);
    if (C == 4 && (reinterpret_cast<uintptr_t>(probs) & 15) == 0)
        hipLaunchKernelGGL(probs_to_labels4_kernel, dim3(grid), dim3(256), 0, c->stream, reinterpret_cast<const float4*>(probs), V, lut, labels);
    else
        hipLaunchKernelGGL(probs_to_labels_kernel, dim3(grid), dim3(256), 0, c->stream, probs, V, (int)C, lut, labels);
    PS_HIP(hipGetLastError());
    return PS_OK;
}

extern "C" int64_t ps_seg_metrics_scratch_bytes(int64_t D0, int64_t D1, int64_t D2, int32_t R)
{
    if (D0 < 1 || D1 < 1 || D2 < 1 || R < 1 || R > kMetricRegions) return -1;
    return (int64_t)seg_scratch_bytes(D0 * D1 * D2, R);
}

extern "C" int ps_seg_metrics(ps_context* c, const uint8_t* pred, const uint8_t* truth, int64_t D0, int64_t D1, int64_t D2, const double* spacing,
                              const uint32_t* regions, int32_t R, void* scratch, int64_t scratch_bytes, int64_t* counts, double* scores)
{
    PS_CHECK(c && pred && truth && spacing && regions && scratch && counts && scores, "ps_seg_metrics: NULL argument");
    PS_CHECK(R >= 1 && R <= kMetricRegions, "ps_seg_metrics: R must be in [1, %d] (got %d)", kMetricRegions, R);
    PS_CHECK(D0 >= 1 && D1 >= 1 && D2 >= 1 && D0 * D1 * D2 < (1ll << 31), "ps_seg_metrics: bad volume shape");
    const int64_t D[3] = {D0, D1, D2};
    for (int a = 0; a < 3; ++a) {
        PS_CHECK(D[a] <= kEdtLineElems, "ps_seg_metrics: axis %d has %lld voxels (limit %d)", a, (long long)D[a], kEdtLineElems);
        PS_CHECK(std::isfinite(spacing[a]) && spacing[a] > 0.0, "ps_seg_metrics: spacing[%d] must be finite and > 0", a);
    }
    const int64_t V = D0 * D1 * D2;
    PS_CHECK(scratch_bytes >= (int64_t)seg_scratch_bytes(V, R), "ps_seg_metrics: scratch holds %lld bytes, %lld needed (ps_seg_metrics_scratch_bytes)",
             (long long)scratch_bytes, (long long)seg_scratch_bytes(V, R));
    PS_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    char* base = static_cast<char*>(scratch);
    SegState* st = reinterpret_cast<SegState*>(base);
    uint16_t* flags = reinterpret_cast<uint16_t*>(base + al256(sizeof(SegState)));
    double* edt = reinterpret_cast<double*>(base + al256(sizeof(SegState)) + al256((size_t)V * 2));
    SegGeom g;
    for (int a = 0; a < 3; ++a) g.d[a] = (int)D[a];
    g.s[2] = 1;
    g.s[1] = (int)D2;
    g.s[0] = (int)(D1 * D2);
    g.V = (int)V;
    RegionTable reg = {};
    for (int r = 0; r < R; ++r) reg.m[r] = regions[r];
    Stage stg(c, "seg_metrics", 21);
    PS_HIP(hipMemsetAsync(st, 0, sizeof(SegState), s));
    const int grid = std::min(ceil_div(V, 256), 2048);
    hipLaunchKernelGGL(seg_mask_kernel, dim3(grid), dim3(256), 0, s, pred, truth, g, (int)R, reg, flags, st);
    // EDT: the contiguous axis first (from the flags), then axis 1, then axis 0 at the read voxels only
    const int order[3] = {2, 1, 0};
    for (int p = 0; p < 3; ++p) {
        const int a = order[p];
        const int b = a == 2 ? 1 : 2, cc = a == 0 ? 1 : 0;
        const int L = (int)D[a];
        const int G = std::max(1, std::min(kEdtMaxLines, kEdtLineElems / L));
        const long long lines = D[b] * D[cc];  // (< 2^31)
        const size_t smem = (((size_t)G * L + 1) & ~(size_t)1) * sizeof(double) + (size_t)G * L * 2 * sizeof(double);
        const dim3 eg((unsigned)((lines + G - 1) / G), (unsigned)(2 * R));
        const void* kern = p == 0 ? reinterpret_cast<const void*>(edt_pass_kernel<true, false>)
                                  : p == 1 ? reinterpret_cast<const void*>(edt_pass_kernel<false, false>)
                                           : reinterpret_cast<const void*>(edt_pass_kernel<false, true>);
        if (smem > 48 * 1024) PS_HIP(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
        if (p == 0) hipLaunchKernelGGL((edt_pass_kernel<true, false>), eg, dim3(256), smem, s, edt, flags, g, a, b, cc, G, spacing[a]);
        else if (p == 1) hipLaunchKernelGGL((edt_pass_kernel<false, false>), eg, dim3(256), smem, s, edt, flags, g, a, b, cc, G, spacing[a]);
        else hipLaunchKernelGGL((edt_pass_kernel<false, true>), eg, dim3(256), smem, s, edt, flags, g, a, b, cc, G, spacing[a]);
    }
    hipLaunchKernelGGL(seg_rank_kernel, dim3(1), dim3(64), 0, s, st, (int)R);
    for (int shift = 56; shift >= 0; shift -= 8) {
        hipLaunchKernelGGL(seg_select_hist_kernel, dim3(grid), dim3(256), 0, s, edt, flags, (int)V, (int)R, shift, st);
        hipLaunchKernelGGL(seg_select_pick_kernel, dim3(1), dim3(64), 0, s, st, (int)R, shift);
    }
    hipLaunchKernelGGL(seg_finish_kernel, dim3(1), dim3(64), 0, s, st, (int)R);
    PS_HIP(hipGetLastError());
    long long h_counts[kMetricRegions][3];
    double h_scores[kMetricRegions][2];
    PS_HIP(hipMemcpyAsync(h_counts, st->out_counts, sizeof(h_counts), hipMemcpyDeviceToHost, s));
    PS_HIP(hipMemcpyAsync(h_scores, st->out_scores, sizeof(h_scores), hipMemcpyDeviceToHost, s));
    PS_HIP(hipStreamSynchronize(s));
    for (int r = 0; r < R; ++r) {
        for (int k = 0; k < 3; ++k) counts[3 * r + k] = h_counts[r][k];
        scores[2 * r] = h_scores[r][0];
        scores[2 * r + 1] = h_scores[r][1];
    }
    return PS_OK;
}
