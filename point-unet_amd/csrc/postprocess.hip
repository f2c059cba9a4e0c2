// postprocess.hip -- the clean-up of a predicted label volume (include/pointseg_postprocess.h): 3-D connected components, binary
// morphology, component selection, hole filling and the BraTS chain built from them.  The rules are the header's, restated in numpy by
// tests/postprocess_ref.py.
//
// Connected components ("Label clean-up"): union-find over the parent array P[V] with root = the smallest linear index.
//   1. cc_tile_kernel      one workgroup labels a kT0 x kT1 x kT2 tile in LDS (local indices grow with the linear index, so the local
//                          root is the tile's smallest voxel of the component) and writes P[v] = the root's linear index, -1 outside the set
//   2. cc_merge_kernel     every voxel unites itself with its neighbours in other tiles -- face, edge- and corner-diagonal -- with
//                          atomicMin on P
//   3. cc_compress_kernel  P[v] = root, and per root: voxel count and face flag (C), overlap count or root flag (R), the number of roots
// No workgroup waits for another.  A parent only ever decreases (every write to P is an atomicMin with a smaller index of the same
// component, or the root itself), so every find / union loop ends; a stale read of P yields an older, larger ancestor of the same
// component, and the atomicMin's return value -- the truth -- decides whether a union is done.
#include <algorithm>

#include "../../include/pointseg_postprocess.h"
#include "common.h"
#include "scratch.h"
#include "sortscan.h"

namespace ps {

namespace {

constexpr int kT0 = 4, kT1 = 8, kT2 = 64;  // the LDS tile; kT2 = one wave of contiguous bytes per row
constexpr int kTileVox = kT0 * kT1 * kT2;
constexpr unsigned kFaceBit = 0x80000000u;  // of C[root]: the component has a voxel on a face of the array (sizes are < 2^31)

struct PpDims {
    int d0, d1, d2;
    int V;
};

// how a byte volume is read as a set: all != 0: (b & mask) == mask, otherwise (b & mask) != 0; flipped when invert != 0
struct PpRead {
    const uint8_t* p;
    unsigned mask;
    int all, invert;
    __device__ __forceinline__ bool test(int v) const
    {
        const unsigned b = p[v] & mask;
        return (all ? b == mask : b != 0u) != (invert != 0);
    }
};

// counters of one component run; zeroed by a memset in front of it
struct CcStat {
    int n;                           // components
    int count;                       // voxels the apply kernel counted (the chain's whole / enhancing counts)
    unsigned long long best1, best2;  // PS_KEEP_LARGEST_TWO: (size << 32) | ~root of the largest and of the second largest
};

__device__ __forceinline__ bool pp_neighbour(int e0, int e1, int e2, int conn)
{
    const int k = (e0 != 0) + (e1 != 0) + (e2 != 0);
    return k != 0 && k <= conn;
}

// ---- union-find ----------------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ int lds_find(const volatile int* P, int x)
{
    int p = P[x];
    while (p != x) {
        x = p;
        p = P[x];
    }
    return x;
}

__device__ __forceinline__ void lds_union(int* P, int a, int b)
{
    bool done = false;
    while (!done) {
        a = lds_find(P, a);
        b = lds_find(P, b);
        if (a == b) break;
        if (a > b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(&P[b], a);  // a < b: the parent of b only decreases
        done = old == b;
        b = old;
    }
}

__device__ __forceinline__ int gl_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int gl_find(const int* P, int x)
{
    int p = gl_load(P + x);
    while (p != x) {
        x = p;
        p = gl_load(P + x);
    }
    return x;
}

__device__ __forceinline__ void gl_union(int* P, int a, int b)
{
    bool done = false;
    while (!done) {
        a = gl_find(P, a);
        b = gl_find(P, b);
        if (a == b) break;
        if (a > b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(&P[b], a);
        done = old == b;
        b = old;
    }
}

__global__ __launch_bounds__(256) void cc_tile_kernel(PpRead in, PpDims d, int conn, int nt1, int nt2, int* __restrict__ P, int* __restrict__ C,
                                                      int* __restrict__ R)
{
    __shared__ int par[kTileVox];
    const int tile = blockIdx.x;
    const int o2 = (tile % nt2) * kT2, o1 = (tile / nt2 % nt1) * kT1, o0 = (tile / nt2 / nt1) * kT0;
#pragma unroll
    for (int k = 0; k < kTileVox / 256; ++k) {
        const int li = k * 256 + threadIdx.x;
        const int g2 = o2 + (li % kT2), g1 = o1 + (li / kT2 % kT1), g0 = o0 + li / (kT2 * kT1);
        const bool inside = g0 < d.d0 && g1 < d.d1 && g2 < d.d2;
        par[li] = inside && in.test((g0 * d.d1 + g1) * d.d2 + g2) ? li : -1;
    }
    __syncthreads();
    // every voxel unites itself with the neighbours of the tile that precede it (each pair once)
#pragma unroll 1
    for (int k = 0; k < kTileVox / 256; ++k) {
        const int li = k * 256 + threadIdx.x;
        if (par[li] < 0) continue;
        const int l2 = li % kT2, l1 = li / kT2 % kT1, l0 = li / (kT2 * kT1);
        for (int e0 = -1; e0 <= 0; ++e0)
            for (int e1 = -1; e1 <= (e0 < 0 ? 1 : 0); ++e1)
                for (int e2 = -1; e2 <= (e0 < 0 || e1 < 0 ? 1 : -1); ++e2) {
                    if (!pp_neighbour(e0, e1, e2, conn)) continue;
                    const int m0 = l0 + e0, m1 = l1 + e1, m2 = l2 + e2;
                    if (m0 < 0 || m1 < 0 || m1 >= kT1 || m2 < 0 || m2 >= kT2) continue;
                    const int lj = (m0 * kT1 + m1) * kT2 + m2;
                    if (par[lj] >= 0) lds_union(par, li, lj);
                }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kTileVox / 256; ++k) {
        const int li = k * 256 + threadIdx.x;
        const int g2 = o2 + (li % kT2), g1 = o1 + (li / kT2 % kT1), g0 = o0 + li / (kT2 * kT1);
        if (g0 >= d.d0 || g1 >= d.d1 || g2 >= d.d2) continue;
        const int v = (g0 * d.d1 + g1) * d.d2 + g2;
        int root = -1;
        if (par[li] >= 0) {
            const int r = lds_find(par, li);
            root = ((o0 + r / (kT2 * kT1)) * d.d1 + o1 + (r / kT2 % kT1)) * d.d2 + o2 + (r % kT2);
        }
        P[v] = root;
        C[v] = 0;
        if (R) R[v] = 0;
    }
}

__global__ __launch_bounds__(256) void cc_merge_kernel(PpDims d, int conn, int* __restrict__ P)
{
    const unsigned v = blockIdx.x * 256u + threadIdx.x;
    if (v >= (unsigned)d.V) return;
    if (P[v] < 0) return;  // (the sign of an entry never changes)
    const int g2 = v % d.d2, g1 = v / d.d2 % d.d1, g0 = v / d.d2 / d.d1;
    const int l0 = g0 % kT0, l1 = g1 % kT1, l2 = g2 % kT2;
    if (l0 != 0 && l1 != 0 && l1 != kT1 - 1 && l2 != 0 && l2 != kT2 - 1) return;  // no preceding neighbour in another tile
    for (int e0 = -1; e0 <= 0; ++e0)
        for (int e1 = -1; e1 <= (e0 < 0 ? 1 : 0); ++e1)
            for (int e2 = -1; e2 <= (e0 < 0 || e1 < 0 ? 1 : -1); ++e2) {
                if (!pp_neighbour(e0, e1, e2, conn)) continue;
                const int m0 = g0 + e0, m1 = g1 + e1, m2 = g2 + e2;
                if (m0 < 0 || m1 < 0 || m1 >= d.d1 || m2 < 0 || m2 >= d.d2) continue;
                const int t0 = l0 + e0, t1 = l1 + e1, t2 = l2 + e2;
                if (t0 >= 0 && t1 >= 0 && t1 < kT1 && t2 >= 0 && t2 < kT2) continue;  // same tile: united in LDS
                const int w = (m0 * d.d1 + m1) * d.d2 + m2;
                if (P[w] >= 0) gl_union(P, (int)v, w);
            }
}

// the lanes of a wave hold consecutive voxels, which mostly share a root: one atomic per run of equal roots
struct WaveRun {
    bool head;
    unsigned long long span;  // the run's lanes
};
__device__ __forceinline__ WaveRun wave_run(int key, int lane)
{
    const int prev = __shfl_up(key, 1);
    const bool head = lane == 0 || prev != key;
    const unsigned long long heads = __ballot(head);
    const unsigned long long rest = lane == 63 ? 0ull : heads >> (lane + 1);
    const int len = rest ? __ffsll((long long)rest) : 64 - lane;
    const unsigned long long ones = len == 64 ? ~0ull : (1ull << len) - 1ull;
    return {head, ones << lane};
}

// mode 0: R untouched; 1: R[v] = (v is a root), the input of the numbering scan; 2: R[root] = voxels of the component set in `main`
__global__ __launch_bounds__(256) void cc_compress_kernel(PpDims d, int* __restrict__ P, int* __restrict__ C, int* __restrict__ R, int mode,
                                                          const uint8_t* __restrict__ main, CcStat* __restrict__ st)
{
    const unsigned v = blockIdx.x * 256u + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool in_vol = v < (unsigned)d.V;
    int root = -1;
    if (in_vol && P[v] >= 0) {
        const int p = gl_load(P + v);
        root = gl_find(P, p);
        if (p != root) {
            atomicMin(&P[p], root);  // shorten the chain above the tile's root for the voxels behind it
            atomicMin(&P[v], root);
        }
    }
    bool face = false, over = false;
    if (root >= 0) {
        const int g2 = v % d.d2, g1 = v / d.d2 % d.d1, g0 = v / d.d2 / d.d1;
        face = g0 == 0 || g1 == 0 || g2 == 0 || g0 == d.d0 - 1 || g1 == d.d1 - 1 || g2 == d.d2 - 1;
        over = mode == 2 && main[v] != 0;
    }
    const bool is_root = root == (int)v && in_vol;
    if (mode == 1 && in_vol) R[v] = is_root ? 1 : 0;
    const WaveRun run = wave_run(root, lane);
    const unsigned long long faces = __ballot(face), overs = __ballot(over), roots = __ballot(is_root);
    if (run.head && root >= 0) {
        atomicAdd(&C[root], __popcll(run.span));
        if (faces & run.span) atomicOr(reinterpret_cast<unsigned*>(&C[root]), kFaceBit);
        if (overs & run.span) atomicAdd(&R[root], __popcll(overs & run.span));
    }
    if (lane == 0 && roots) atomicAdd(&st->n, __popcll(roots));
}

// after the scan of the root flags: R[root] = the component's number - 1
__global__ __launch_bounds__(256) void cc_number_kernel(PpDims d, const int* __restrict__ P, const int* __restrict__ C, const int* __restrict__ R,
                                                        const CcStat* __restrict__ st, int* __restrict__ labels, int* __restrict__ n,
                                                        int* __restrict__ sizes, uint8_t* __restrict__ touches)
{
    const unsigned v = blockIdx.x * 256u + threadIdx.x;
    if (v == 0) *n = st->n;
    if (v >= (unsigned)d.V) return;
    const int root = P[v];
    labels[v] = root >= 0 ? R[root] + 1 : 0;
    if (root == (int)v) {
        const unsigned c = (unsigned)C[v];
        if (sizes) sizes[R[v]] = (int)(c & ~kFaceBit);
        if (touches) touches[R[v]] = (c & kFaceBit) ? 1 : 0;
    }
}

// PS_KEEP_LARGEST_TWO: the largest key over the roots; pass 1 leaves out the winner of pass 0
__global__ __launch_bounds__(256) void cc_top_kernel(PpDims d, const int* __restrict__ P, const int* __restrict__ C, CcStat* __restrict__ st, int pass)
{
    const unsigned v = blockIdx.x * 256u + threadIdx.x;
    unsigned long long key = 0;
    if (v < (unsigned)d.V && P[v] == (int)v) {
        key = ((unsigned long long)((unsigned)C[v] & ~kFaceBit) << 32) | (unsigned long long)(~v);
        if (pass == 1 && key == st->best1) key = 0;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const unsigned long long other = __shfl_xor(key, o);
        key = other > key ? other : key;
    }
    if ((threadIdx.x & 63) == 0 && key) atomicMax(pass == 0 ? &st->best1 : &st->best2, key);
}

// what a finished component run keeps
struct PpKeep {
    int rule;  // PS_KEEP_*, or 0: the components that touch no face (hole filling)
    long long threshold;
};

// dst[v] = (dst[v] & keep_mask) | (kept ? set_bits : 0) | (base set at v ? base_bits : 0); counts the voxels whose new byte has all of count_mask
__global__ __launch_bounds__(256) void cc_apply_kernel(PpDims d, const int* __restrict__ P, const int* __restrict__ C, const int* __restrict__ R,
                                                       CcStat* __restrict__ st, PpKeep k, PpRead base, unsigned base_bits, uint8_t* __restrict__ dst,
                                                       unsigned keep_mask, unsigned set_bits, unsigned count_mask)
{
    const unsigned v = blockIdx.x * 256u + threadIdx.x;
    bool counted = false;
    if (v < (unsigned)d.V) {
        const int root = P[v];
        bool kept = false;
        if (root >= 0) {
            const unsigned c = (unsigned)C[root];
            const long long size = (long long)(c & ~kFaceBit);
            if (k.rule == PS_KEEP_ABOVE) {
                kept = st->n == 1 || size > k.threshold;
            } else if (k.rule == PS_KEEP_LARGEST_TWO) {
                const unsigned long long b1 = st->best1, b2 = st->best2;
                const unsigned r1 = ~(unsigned)b1, r2 = ~(unsigned)b2;
                kept = st->n <= 1 || (unsigned)root == r1 || (b2 != 0 && (unsigned)root == r2 && 10ull * (b2 >> 32) > (b1 >> 32));
            } else if (k.rule == PS_KEEP_OVERLAP) {
                kept = 2ll * (long long)R[root] >= size;
            } else {
                kept = !(c & kFaceBit);
            }
        }
        unsigned b = keep_mask ? dst[v] & keep_mask : 0u;
        if (kept) b |= set_bits;
        if (base.p && base.test((int)v)) b |= base_bits;
        dst[v] = (uint8_t)b;
        counted = count_mask && (b & count_mask) == count_mask;
    }
    const unsigned long long cnt = __ballot(counted);
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(&st->count, __popcll(cnt));
}

// ---- morphology ----------------------------------------------------------------------------------------------------------------------------
// One round: dst[v] = (dst[v] & keep_mask) | (result ? set_bits : 0).  In place (src.p == dst) the round reads one bit plane and writes
// another, as vs_dilate_kernel (volume_sample.hip) does: keep_mask holds the plane being read, so the byte a neighbour reads never
// changes in the bits it looks at.
template <bool ERODE>
__global__ __launch_bounds__(256) void pp_morph_kernel(PpRead src, PpDims d, int conn, uint8_t* __restrict__ dst, unsigned keep_mask, unsigned set_bits)
{
    const unsigned v = blockIdx.x * 256u + threadIdx.x;
    if (v >= (unsigned)d.V) return;
    const int g2 = v % d.d2, g1 = v / d.d2 % d.d1, g0 = v / d.d2 / d.d1;
    bool r = src.test((int)v);
    if (r == ERODE) {  // a dilation of a set voxel and an erosion of a clear one are decided
        for (int e0 = -1; e0 <= 1; ++e0)
            for (int e1 = -1; e1 <= 1; ++e1)
                for (int e2 = -1; e2 <= 1; ++e2) {
                    if (!pp_neighbour(e0, e1, e2, conn)) continue;
                    const int m0 = g0 + e0, m1 = g1 + e1, m2 = g2 + e2;
                    const bool inside = m0 >= 0 && m0 < d.d0 && m1 >= 0 && m1 < d.d1 && m2 >= 0 && m2 < d.d2;
                    const bool s = inside && src.test((m0 * d.d1 + m1) * d.d2 + m2);  // outside the array: 0, for both
                    if (ERODE) r = r && s;
                    else r = r || s;
                }
    }
    dst[v] = (uint8_t)((keep_mask ? dst[v] & keep_mask : 0u) | (r ? set_bits : 0u));
}

void morph_round(hipStream_t sm, bool erode, const PpRead& src, const PpDims& d, int conn, uint8_t* dst, unsigned keep_mask, unsigned set_bits)
{
    if (erode) hipLaunchKernelGGL(pp_morph_kernel<true>, dim3(blocks256((size_t)d.V)), dim3(256), 0, sm, src, d, conn, dst, keep_mask, set_bits);
    else hipLaunchKernelGGL(pp_morph_kernel<false>, dim3(blocks256((size_t)d.V)), dim3(256), 0, sm, src, d, conn, dst, keep_mask, set_bits);
}

// whole / core / enhancing of the chain as bits 2 / 3 / 4 of the work volume (bits 0 and 1 are the planes of the morphology rounds)
constexpr unsigned kWhole = 4u, kCore = 8u, kEnh = 16u;

__global__ __launch_bounds__(256) void brats_split_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ weight, int V, uint8_t* __restrict__ W)
{
    const unsigned v = blockIdx.x * 256u + threadIdx.x;
    if (v >= (unsigned)V) return;
    const unsigned p = weight && weight[v] == 0 ? 0u : pred[v];
    W[v] = (uint8_t)((p > 0 ? kWhole : 0u) | (p > 0 && p != 2 ? kCore : 0u) | (p == 4 ? kEnh : 0u));
}

// st[0].count = count(whole), st[1].count = count(enh & core): the small-enhancing-region rule is decided here, by every thread alike
__global__ __launch_bounds__(256) void brats_join_kernel(const uint8_t* __restrict__ W, int V, const CcStat* __restrict__ st, uint8_t* __restrict__ out)
{
    const unsigned v = blockIdx.x * 256u + threadIdx.x;
    if (v >= (unsigned)V) return;
    const int whole = st[0].count, enh = st[1].count;
    const bool clear_enh = whole > 100 && enh > 0 && enh < 100;
    const unsigned b = W[v];
    unsigned o = (b & kWhole) ? 2u : 0u;
    if (b & kCore) o = 1u;
    if ((b & (kCore | kEnh)) == (kCore | kEnh) && !clear_enh) o = 4u;
    out[v] = (uint8_t)o;
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------------

int check_dims(const char* who, int64_t d0, int64_t d1, int64_t d2, PpDims* d)
{
    const int64_t lim = 1ll << 31;
    PS_CHECK(d0 >= 1 && d1 >= 1 && d2 >= 1 && d0 < lim && d1 < lim && d2 < lim && d0 * d1 < lim && d0 * d1 * d2 < lim,
             "%s: volume %lld x %lld x %lld (every dimension >= 1, d0 * d1 * d2 < 2^31)", who, (long long)d0, (long long)d1, (long long)d2);
    *d = {(int)d0, (int)d1, (int)d2, (int)(d0 * d1 * d2)};
    return PS_OK;
}

int check_connectivity(const char* who, int32_t connectivity)
{
    PS_CHECK(connectivity >= 1 && connectivity <= 3, "%s: connectivity = %d, must be 1, 2 or 3", who, (int)connectivity);
    return PS_OK;
}

// launches 1-3 of the header comment: 3 kernels.  R may be nullptr with mode 0.
void cc_run(hipStream_t sm, const PpRead& in, const PpDims& d, int conn, int* P, int* C, int* R, int mode, const uint8_t* main, CcStat* st)
{
    const int nt0 = ceil_div(d.d0, kT0), nt1 = ceil_div(d.d1, kT1), nt2 = ceil_div(d.d2, kT2);
    const dim3 vgrid(blocks256((size_t)d.V));
    hipLaunchKernelGGL(cc_tile_kernel, dim3((unsigned)((size_t)nt0 * nt1 * nt2)), dim3(256), 0, sm, in, d, conn, nt1, nt2, P, C, R);
    hipLaunchKernelGGL(cc_merge_kernel, vgrid, dim3(256), 0, sm, d, conn, P);
    hipLaunchKernelGGL(cc_compress_kernel, vgrid, dim3(256), 0, sm, d, P, C, R, mode, main, st);
}

void cc_apply(hipStream_t sm, const PpDims& d, const int* P, const int* C, const int* R, CcStat* st, const PpKeep& k, const PpRead& base,
              unsigned base_bits, uint8_t* dst, unsigned keep_mask, unsigned set_bits, unsigned count_mask)
{
    hipLaunchKernelGGL(cc_apply_kernel, dim3(blocks256((size_t)d.V)), dim3(256), 0, sm, d, P, C, R, st, k, base, base_bits, dst, keep_mask, set_bits,
                       count_mask);
}

constexpr size_t kStatBytes = 256;
static_assert(2 * sizeof(CcStat) <= kStatBytes, "the counters of the chain's two component runs");

}  // namespace

}  // namespace ps

extern "C" int ps_label_components(ps_context* c, const void* volume, int64_t d0, int64_t d1, int64_t d2, int32_t connectivity, int32_t background,
                                   void* labels, void* n, void* sizes, void* touches, void* scratch, int64_t* scratch_bytes)
{
    using namespace ps;
    static const char* who = "ps_label_components";
    PS_CHECK(scratch_bytes && (c || !scratch), "%s: NULL argument", who);
    PS_CHECK(!scratch || (volume && labels && n), "%s: NULL volume, labels or n (they may be NULL only in the call that sizes the scratch)", who);
    PpDims d;
    PS_TRY(check_dims(who, d0, d1, d2, &d));
    PS_TRY(check_connectivity(who, connectivity));
    PS_CHECK(background == 0 || background == 1, "%s: background = %d, must be 0 or 1", who, (int)background);
    Carver cv{static_cast<char*>(scratch)};
    CcStat* st = cv.take<CcStat>(kStatBytes / sizeof(CcStat));
    int* P = cv.take<int>((size_t)d.V);
    int* C = cv.take<int>((size_t)d.V);
    int* R = cv.take<int>((size_t)d.V);
    unsigned* work = cv.take<unsigned>(scan_workspace_words((size_t)d.V));
    if (!scratch) {
        *scratch_bytes = (int64_t)cv.off;
        return PS_OK;
    }
    PS_TRY(check_scratch(who, scratch, scratch_bytes, cv.off));

    PS_HIP(hipSetDevice(c->device));
    hipStream_t sm = c->stream;
    Stage stg(c, "label_components", 4 + scan_launches((size_t)d.V));
    PS_HIP(hipMemsetAsync(st, 0, kStatBytes, sm));
    const PpRead in = {static_cast<const uint8_t*>(volume), 0xffu, 0, background};
    cc_run(sm, in, d, connectivity, P, C, R, 1, nullptr, st);
    exclusive_scan_u32(sm, reinterpret_cast<unsigned*>(R), reinterpret_cast<unsigned*>(R), (size_t)d.V, work);
    hipLaunchKernelGGL(cc_number_kernel, dim3(blocks256((size_t)d.V)), dim3(256), 0, sm, d, P, C, R, st, static_cast<int*>(labels), static_cast<int*>(n),
                       static_cast<int*>(sizes), static_cast<uint8_t*>(touches));
    PS_HIP(hipGetLastError());
    return PS_OK;
}

extern "C" int ps_binary_morph(ps_context* c, const void* in, int64_t d0, int64_t d1, int64_t d2, int32_t op, int32_t connectivity, int32_t iterations,
                               void* out, void* scratch, int64_t* scratch_bytes)
{
    using namespace ps;
    static const char* who = "ps_binary_morph";
    PS_CHECK(scratch_bytes && (c || !scratch), "%s: NULL argument", who);
    PS_CHECK(!scratch || (in && out), "%s: NULL volume (in and out may be NULL only in the call that sizes the scratch)", who);
    PpDims d;
    PS_TRY(check_dims(who, d0, d1, d2, &d));
    PS_TRY(check_connectivity(who, connectivity));
    PS_CHECK(op >= PS_MORPH_DILATE && op <= PS_MORPH_OPEN, "%s: op = %d is none of PS_MORPH_DILATE, _ERODE, _CLOSE, _OPEN", who, (int)op);
    PS_CHECK(iterations >= 1 && iterations <= (1 << 20), "%s: iterations = %d, must be in [1, 2^20]", who, (int)iterations);
    Carver cv{static_cast<char*>(scratch)};
    uint8_t* W = cv.take<uint8_t>((size_t)d.V);
    if (!scratch) {
        *scratch_bytes = (int64_t)cv.off;
        return PS_OK;
    }
    PS_TRY(check_scratch(who, scratch, scratch_bytes, cv.off));
    PS_CHECK(in != out, "%s: in and out must not overlap", who);

    PS_HIP(hipSetDevice(c->device));
    hipStream_t sm = c->stream;
    const int rounds = (op == PS_MORPH_CLOSE || op == PS_MORPH_OPEN ? 2 : 1) * iterations;
    Stage stg(c, "binary_morph", rounds);
    // round 0 reads `in`, the last round writes `out` as 0 / 1; the rounds between alternate between bits 0 and 1 of W
    for (int r = 0; r < rounds; ++r) {
        const bool second = r >= iterations;
        const bool erode = op == PS_MORPH_ERODE || (op == PS_MORPH_CLOSE && second) || (op == PS_MORPH_OPEN && !second);
        const PpRead src = r == 0 ? PpRead{static_cast<const uint8_t*>(in), 0xffu, 0, 0} : PpRead{W, 1u << ((r - 1) & 1), 0, 0};
        if (r == rounds - 1) morph_round(sm, erode, src, d, connectivity, static_cast<uint8_t*>(out), 0u, 1u);
        else morph_round(sm, erode, src, d, connectivity, W, r == 0 ? 0u : src.mask, 1u << (r & 1));
    }
    PS_HIP(hipGetLastError());
    return PS_OK;
}

extern "C" int ps_keep_components(ps_context* c, const void* mask, int64_t d0, int64_t d1, int64_t d2, int32_t connectivity, int32_t rule,
                                  int64_t threshold, const void* main, void* out, void* scratch, int64_t* scratch_bytes)
{
    using namespace ps;
    static const char* who = "ps_keep_components";
    PS_CHECK(scratch_bytes && (c || !scratch), "%s: NULL argument", who);
    PS_CHECK(!scratch || (mask && out), "%s: NULL volume (mask and out may be NULL only in the call that sizes the scratch)", who);
    PpDims d;
    PS_TRY(check_dims(who, d0, d1, d2, &d));
    PS_TRY(check_connectivity(who, connectivity));
    PS_CHECK(rule == PS_KEEP_ABOVE || rule == PS_KEEP_LARGEST_TWO || rule == PS_KEEP_OVERLAP,
             "%s: rule = %d is none of PS_KEEP_ABOVE, PS_KEEP_LARGEST_TWO, PS_KEEP_OVERLAP", who, (int)rule);
    PS_CHECK(rule != PS_KEEP_ABOVE || threshold >= 0, "%s: threshold = %lld, must be >= 0", who, (long long)threshold);
    PS_CHECK(!scratch || rule != PS_KEEP_OVERLAP || main, "%s: PS_KEEP_OVERLAP needs main", who);
    Carver cv{static_cast<char*>(scratch)};
    CcStat* st = cv.take<CcStat>(kStatBytes / sizeof(CcStat));
    int* P = cv.take<int>((size_t)d.V);
    int* C = cv.take<int>((size_t)d.V);
    int* R = rule == PS_KEEP_OVERLAP ? cv.take<int>((size_t)d.V) : nullptr;
    if (!scratch) {
        *scratch_bytes = (int64_t)cv.off;
        return PS_OK;
    }
    PS_TRY(check_scratch(who, scratch, scratch_bytes, cv.off));
    PS_CHECK(mask != out && main != out, "%s: mask, main and out must not overlap", who);

    PS_HIP(hipSetDevice(c->device));
    hipStream_t sm = c->stream;
    Stage stg(c, "keep_components", rule == PS_KEEP_LARGEST_TWO ? 6 : 4);
    PS_HIP(hipMemsetAsync(st, 0, kStatBytes, sm));
    const PpRead in = {static_cast<const uint8_t*>(mask), 0xffu, 0, 0};
    cc_run(sm, in, d, connectivity, P, C, R, rule == PS_KEEP_OVERLAP ? 2 : 0, static_cast<const uint8_t*>(main), st);
    if (rule == PS_KEEP_LARGEST_TWO)
        for (int pass = 0; pass < 2; ++pass) hipLaunchKernelGGL(cc_top_kernel, dim3(blocks256((size_t)d.V)), dim3(256), 0, sm, d, P, C, st, pass);
    cc_apply(sm, d, P, C, R, st, PpKeep{rule, (long long)threshold}, PpRead{nullptr, 0u, 0, 0}, 0u, static_cast<uint8_t*>(out), 0u, 1u, 0u);
    PS_HIP(hipGetLastError());
    return PS_OK;
}

extern "C" int ps_fill_holes(ps_context* c, const void* mask, int64_t d0, int64_t d1, int64_t d2, void* out, void* scratch, int64_t* scratch_bytes)
{
    using namespace ps;
    static const char* who = "ps_fill_holes";
    PS_CHECK(scratch_bytes && (c || !scratch), "%s: NULL argument", who);
    PS_CHECK(!scratch || (mask && out), "%s: NULL volume (mask and out may be NULL only in the call that sizes the scratch)", who);
    PpDims d;
    PS_TRY(check_dims(who, d0, d1, d2, &d));
    Carver cv{static_cast<char*>(scratch)};
    CcStat* st = cv.take<CcStat>(kStatBytes / sizeof(CcStat));
    int* P = cv.take<int>((size_t)d.V);
    int* C = cv.take<int>((size_t)d.V);
    if (!scratch) {
        *scratch_bytes = (int64_t)cv.off;
        return PS_OK;
    }
    PS_TRY(check_scratch(who, scratch, scratch_bytes, cv.off));
    PS_CHECK(mask != out, "%s: mask and out must not overlap", who);

    PS_HIP(hipSetDevice(c->device));
    hipStream_t sm = c->stream;
    Stage stg(c, "fill_holes", 4);
    PS_HIP(hipMemsetAsync(st, 0, kStatBytes, sm));
    // the 6-connected components of the zero voxels; the ones that touch no face are the holes
    const PpRead zeros = {static_cast<const uint8_t*>(mask), 0xffu, 0, 1}, set = {static_cast<const uint8_t*>(mask), 0xffu, 0, 0};
    cc_run(sm, zeros, d, 1, P, C, nullptr, 0, nullptr, st);
    cc_apply(sm, d, P, C, nullptr, st, PpKeep{0, 0}, set, 1u, static_cast<uint8_t*>(out), 0u, 1u, 0u);
    PS_HIP(hipGetLastError());
    return PS_OK;
}

extern "C" int ps_brats_postprocess(ps_context* c, const void* pred, const void* weight, int64_t d0, int64_t d1, int64_t d2, int64_t wt_threshold,
                                    void* out, void* scratch, int64_t* scratch_bytes)
{
    using namespace ps;
    static const char* who = "ps_brats_postprocess";
    PS_CHECK(scratch_bytes && (c || !scratch), "%s: NULL argument", who);
    PS_CHECK(!scratch || (pred && out), "%s: NULL volume (pred and out may be NULL only in the call that sizes the scratch)", who);
    PpDims d;
    PS_TRY(check_dims(who, d0, d1, d2, &d));
    PS_CHECK(wt_threshold >= 0, "%s: wt_threshold = %lld, must be >= 0", who, (long long)wt_threshold);
    Carver cv{static_cast<char*>(scratch)};
    CcStat* st = cv.take<CcStat>(kStatBytes / sizeof(CcStat));
    uint8_t* W = cv.take<uint8_t>((size_t)d.V);
    int* P = cv.take<int>((size_t)d.V);
    int* C = cv.take<int>((size_t)d.V);
    if (!scratch) {
        *scratch_bytes = (int64_t)cv.off;
        return PS_OK;
    }
    PS_TRY(check_scratch(who, scratch, scratch_bytes, cv.off));
    PS_CHECK(pred != out && weight != out, "%s: pred, weight and out must not overlap", who);

    PS_HIP(hipSetDevice(c->device));
    hipStream_t sm = c->stream;
    Stage stg(c, "brats_postprocess", 14);
    const dim3 vgrid(blocks256((size_t)d.V));
    const PpKeep above = {PS_KEEP_ABOVE, (long long)wt_threshold};
    const PpRead none = {nullptr, 0u, 0, 0};
    PS_HIP(hipMemsetAsync(st, 0, kStatBytes, sm));
    hipLaunchKernelGGL(brats_split_kernel, vgrid, dim3(256), 0, sm, static_cast<const uint8_t*>(pred), static_cast<const uint8_t*>(weight), d.V, W);
    // whole: close into bit 1, keep the components above the threshold back into the whole bit, counted
    morph_round(sm, false, PpRead{W, kWhole, 1, 0}, d, 2, W, 0xffu & ~1u, 1u);
    morph_round(sm, true, PpRead{W, 1u, 1, 0}, d, 2, W, 0xffu & ~2u, 2u);
    cc_run(sm, PpRead{W, 2u, 1, 0}, d, 2, P, C, nullptr, 0, nullptr, st);
    cc_apply(sm, d, P, C, nullptr, st, above, none, 0u, W, 0xffu & ~kWhole, kWhole, kWhole);
    // core inside whole, the same way; counted: the enhancing voxels inside the kept core
    morph_round(sm, false, PpRead{W, kWhole | kCore, 1, 0}, d, 2, W, 0xffu & ~1u, 1u);
    morph_round(sm, true, PpRead{W, 1u, 1, 0}, d, 2, W, 0xffu & ~2u, 2u);
    cc_run(sm, PpRead{W, 2u, 1, 0}, d, 2, P, C, nullptr, 0, nullptr, st + 1);
    cc_apply(sm, d, P, C, nullptr, st + 1, above, none, 0u, W, 0xffu & ~kCore, kCore, kCore | kEnh);
    hipLaunchKernelGGL(brats_join_kernel, vgrid, dim3(256), 0, sm, W, d.V, st, static_cast<uint8_t*>(out));
    PS_HIP(hipGetLastError());
    return PS_OK;
}
