// cloud_sample.hip -- training batches drawn on the device from clouds that stay resident in HBM: the input generator of
// PointSegment/runBraTS.py:91-130 (every tumour point, a uniform sample of background points up to cfg.num_points, DP.shuffle_idx) as
// the rule include/pointseg.h states for ps_cloud_sample (restated in numpy by tests/cloud_sample_ref.py).
//
// No key array is ever stored: a point's selection and permutation keys are hashes of its index, so every pass reads only the labels.
//   1. select   four rounds of an 8-bit radix select per slot over the 32-bit selection hash of the background points: the hash h* of
//               the (N - P)-th smallest background key, and r_eq = how many background points with hash h* are taken (the lowest
//               indices first, since the index is the key's low half).  Round 0 also counts the positives (P) on the device.
//               (hash32(i * 2654435761 ^ s) is a bijection of i -- odd multiplier, xor, invertible mixer --, so r_eq is 1 for every
//               cloud of fewer than 2^32 points; the compaction does not rely on it.)
//   2. compact  S = positives + background with hash < h* + the first r_eq background points with hash == h*, in ascending index:
//               per-tile counts, a per-slot scan of the tile totals, a ballot-ranked write of (slot << 32 | permutation hash, i).
//   3. sort     stable LSD radix sort of those pairs (sortscan.hip): ties of the permutation hash stay in ascending index.
//   4. gather   idx, labels, xyz and [xyz | modalities] rows, the float rows staged in LDS and written with 16-byte stores.
#include <algorithm>
#include <vector>

#include "common.h"
#include "sample_hash.h"
#include "sample_select.h"
#include "sortscan.h"

namespace ps {

namespace {

constexpr int kThreads = 256;
constexpr int kPerThread = 16;
constexpr int kTile = kThreads * kPerThread;  // points per workgroup of the per-point passes

// per slot, device: the select's state
struct SampleSlot {
    unsigned hist[256];
    unsigned positives;  // counted by round 0
    unsigned need;       // N - positives (0 when the count exceeds N: the batch is then the first N positives' permutation)
    unsigned prefix;     // selection-hash bits found so far; h* after round 3
    unsigned rank;       // 0-based rank left inside the bucket of `prefix`
    unsigned r_eq;       // background points with hash == h* that are taken (after round 3)
    unsigned pad[3];
};

// per slot, host-filled and uploaded
struct SlotInfo {
    long long row0;     // first row of the slot's cloud in the bank
    unsigned n;         // points of the cloud
    unsigned s_sel, s_perm;
    unsigned p_host;    // positives_host[cloud]
    int cloud;
    unsigned pad;
};

__device__ __forceinline__ unsigned wave_sum(unsigned v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (unsigned)__shfl_xor((int)v, o);
    return v;
}

__global__ __launch_bounds__(256) void cloud_sample_init_kernel(SampleSlot* __restrict__ slots, int* __restrict__ status)
{
    SampleSlot& s = slots[blockIdx.x];
    s.hist[threadIdx.x] = 0;
    if (threadIdx.x == 0) {
        s.positives = 0;
        s.need = 0;
        s.prefix = 0;
        s.rank = 0;
        s.r_eq = 0;
        if (blockIdx.x == 0) status[0] = status[1] = status[2] = status[3] = 0;
    }
}

// one round of the select: histogram of digit (hash >> shift) & 255 over the background points whose higher digits equal the prefix;
// round 0 (shift 24) also counts the positives.  grid (tiles, B).
__global__ __launch_bounds__(256) void cloud_sample_hist_kernel(const int32_t* __restrict__ labels, const SlotInfo* __restrict__ info,
                                                                SampleSlot* __restrict__ slots, int shift)
{
    __shared__ unsigned h[256];
    __shared__ unsigned s_pos[4];
    const SlotInfo inf = info[blockIdx.y];
    SampleSlot& sl = slots[blockIdx.y];
    const unsigned t0 = blockIdx.x * (unsigned)kTile;
    if (t0 >= inf.n) return;
    const bool first = shift == 24;
    if (!first && sl.need == 0) return;  // nothing to select
    const unsigned hi_mask = first ? 0u : ~0u << (shift + 8);
    const unsigned want = first ? 0u : (sl.prefix & hi_mask);
    h[threadIdx.x] = 0;
    __syncthreads();
    const int32_t* lab = labels ? labels + inf.row0 : nullptr;
    unsigned pos = 0;
#pragma unroll 4
    for (int j = 0; j < kPerThread; ++j) {
        const unsigned i = t0 + j * kThreads + threadIdx.x;
        if (i >= inf.n) break;
        const bool p = lab && lab[i] > 0;
        pos += p;
        if (p) continue;
        const unsigned x = point_hash(i, inf.s_sel);
        if ((x & hi_mask) == want) atomicAdd(&h[(x >> shift) & 255u], 1u);
    }
    if (first) {
        pos = wave_sum(pos);
        if ((threadIdx.x & 63) == 0) s_pos[threadIdx.x >> 6] = pos;
    }
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(&sl.hist[threadIdx.x], h[threadIdx.x]);
    if (first && threadIdx.x == 0) {
        const unsigned tot = s_pos[0] + s_pos[1] + s_pos[2] + s_pos[3];
        if (tot) atomicAdd(&sl.positives, tot);
    }
}

// the digit whose bucket holds the remaining rank; clears the histogram for the next round.  Round 0 turns the positive count into the
// number of background points to take and compares it with the host's.  grid B, 256 threads (thread = digit).
__global__ __launch_bounds__(256) void cloud_sample_pick_kernel(const SlotInfo* __restrict__ info, SampleSlot* __restrict__ slots,
                                                                int* __restrict__ status, unsigned N, int shift)
{
    __shared__ unsigned s_need, s_rank;
    SampleSlot& sl = slots[blockIdx.x];
    if (threadIdx.x == 0) {
        if (shift == 24) {
            const unsigned P = sl.positives;
            const unsigned need = P > N ? 0u : N - P;
            sl.need = need;
            sl.rank = need ? need - 1 : 0u;
            if (P != info[blockIdx.x].p_host && atomicCAS(&status[0], 0, 1) == 0) {  // the first slot that disagrees reports
                status[1] = (int)blockIdx.x;
                status[2] = (int)P;
                status[3] = (int)info[blockIdx.x].p_host;
            }
        }
        s_need = sl.need;
        s_rank = sl.rank;
    }
    unsigned left;
    if (select_pick_digit(sl.hist, shift, &s_need, &s_rank, &sl.prefix, left)) {
        sl.rank = left;
        if (shift == 0) sl.r_eq = left + 1;
    }
}

// Step 2.  WRITE = false: the tile's counts of definite members (positives, background below h*) and of background points with hash h*
// -> tiles[(2 * slot + 0 / 1) * ntiles + tile].  WRITE = true: the same classification, ranked in ascending index with ballots, plus the
// tile's scanned offsets -> keys / vals at slot * N + position (positions >= N are never written).  grid (tiles, B).
template <bool WRITE>
__global__ __launch_bounds__(256) void cloud_sample_compact_kernel(const int32_t* __restrict__ labels, const SlotInfo* __restrict__ info,
                                                                   const SampleSlot* __restrict__ slots, unsigned* __restrict__ tiles,
                                                                   unsigned ntiles, unsigned N, unsigned long long* __restrict__ keys,
                                                                   unsigned* __restrict__ vals)
{
    __shared__ unsigned s_cd[kPerThread * 4], s_ce[kPerThread * 4];  // per (round, wave): counts, then exclusive offsets
    const int b = blockIdx.y;
    const SlotInfo inf = info[b];
    const unsigned t0 = blockIdx.x * (unsigned)kTile;
    if (t0 >= inf.n) return;
    const unsigned thr = slots[b].prefix, r_eq = slots[b].r_eq;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int32_t* lab = labels ? labels + inf.row0 : nullptr;
    unsigned long long md[kPerThread], me[kPerThread];
#pragma unroll
    for (int j = 0; j < kPerThread; ++j) {
        const unsigned i = t0 + j * kThreads + threadIdx.x;
        bool def = false, eq = false;
        if (i < inf.n) {
            if (lab && lab[i] > 0) {
                def = true;
            } else {
                const unsigned x = point_hash(i, inf.s_sel);
                def = x < thr;
                eq = x == thr && r_eq != 0;
            }
        }
        md[j] = __ballot(def);
        me[j] = __ballot(eq);
        if (lane == 0) {
            s_cd[j * 4 + wave] = (unsigned)__popcll(md[j]);
            s_ce[j * 4 + wave] = (unsigned)__popcll(me[j]);
        }
    }
    __syncthreads();
    if (!WRITE) {
        if (threadIdx.x < 64) {
            const unsigned td = wave_sum(s_cd[threadIdx.x]), te = wave_sum(s_ce[threadIdx.x]);
            if (threadIdx.x == 0) {
                tiles[(size_t)(2 * b) * ntiles + blockIdx.x] = td;
                tiles[(size_t)(2 * b + 1) * ntiles + blockIdx.x] = te;
            }
        }
        return;
    }
    if (threadIdx.x < 64) {  // entry k = 4 j + w is in element order: exclusive scan over the 64 (round, wave) groups
        const unsigned cd = s_cd[threadIdx.x], ce = s_ce[threadIdx.x];
        const unsigned id = wave_inclusive_sum(cd, lane), ie = wave_inclusive_sum(ce, lane);
        s_cd[threadIdx.x] = id - cd;
        s_ce[threadIdx.x] = ie - ce;
    }
    __syncthreads();
    const unsigned base_d = tiles[(size_t)(2 * b) * ntiles + blockIdx.x], base_e = tiles[(size_t)(2 * b + 1) * ntiles + blockIdx.x];
    const unsigned long long below = (1ull << lane) - 1ull;
    unsigned long long* ko = keys + (size_t)b * N;
    unsigned* vo = vals + (size_t)b * N;
    const unsigned long long slot_hi = (unsigned long long)b << 32;
#pragma unroll
    for (int j = 0; j < kPerThread; ++j) {
        const bool def = (md[j] >> lane) & 1ull, eq = (me[j] >> lane) & 1ull;
        if (!def && !eq) continue;
        const unsigned i = t0 + j * kThreads + threadIdx.x;
        const unsigned dpre = base_d + s_cd[j * 4 + wave] + (unsigned)__popcll(md[j] & below);
        const unsigned epre = base_e + s_ce[j * 4 + wave] + (unsigned)__popcll(me[j] & below);
        unsigned pos;
        if (def) {
            pos = dpre + (epre < r_eq ? epre : r_eq);
        } else {
            if (epre >= r_eq) continue;
            pos = dpre + epre;
        }
        if (pos < N) {
            ko[pos] = slot_hi | point_hash(i, inf.s_perm);
            vo[pos] = i;
        }
    }
}

// exclusive scan of the slot's tile totals (both counts), in place.  grid B, 256 threads.
__global__ __launch_bounds__(256) void cloud_sample_tile_scan_kernel(const SlotInfo* __restrict__ info, unsigned* __restrict__ tiles,
                                                                     unsigned ntiles)
{
    __shared__ unsigned s_w[2][4];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned nt = (info[b].n + kTile - 1) / kTile;
    unsigned* td = tiles + (size_t)(2 * b) * ntiles;
    unsigned* te = tiles + (size_t)(2 * b + 1) * ntiles;
    unsigned carry_d = 0, carry_e = 0;
    for (unsigned k0 = 0; k0 < nt; k0 += 256) {
        const unsigned k = k0 + threadIdx.x;
        const unsigned cd = k < nt ? td[k] : 0u, ce = k < nt ? te[k] : 0u;
        const unsigned id = wave_inclusive_sum(cd, lane), ie = wave_inclusive_sum(ce, lane);
        if (lane == 63) {
            s_w[0][wave] = id;
            s_w[1][wave] = ie;
        }
        __syncthreads();
        unsigned od = carry_d + id - cd, oe = carry_e + ie - ce;
        for (int w = 0; w < wave; ++w) {
            od += s_w[0][w];
            oe += s_w[1][w];
        }
        if (k < nt) {
            td[k] = od;
            te[k] = oe;
        }
        carry_d += s_w[0][0] + s_w[0][1] + s_w[0][2] + s_w[0][3];
        carry_e += s_w[1][0] + s_w[1][1] + s_w[1][2] + s_w[1][3];
        __syncthreads();
    }
}

// Step 4: row t of the batch (flat over [B, N]).  The float rows of a workgroup are contiguous in the outputs: staged in LDS, then
// written with 16-byte stores (row t0 * F floats is 16-byte aligned for every F since t0 is a multiple of 256).
__global__ __launch_bounds__(256) void cloud_sample_gather_kernel(const float* __restrict__ xyz, const float* __restrict__ mods, int C,
                                                                  const int32_t* __restrict__ labels, const SlotInfo* __restrict__ info,
                                                                  const unsigned* __restrict__ vals, unsigned N, unsigned total,
                                                                  float* __restrict__ out_xyz, float* __restrict__ out_f,
                                                                  int32_t* __restrict__ out_l, int32_t* __restrict__ out_i)
{
    __shared__ __attribute__((aligned(16))) float s_f[256 * 19];
    __shared__ __attribute__((aligned(16))) float s_x[256 * 3];
    const int F = 3 + C;
    const unsigned t0 = blockIdx.x * 256u, t = t0 + threadIdx.x;
    const unsigned rows = total - t0 < 256u ? total - t0 : 256u;
    if (t < total) {
        const unsigned b = t / N;
        unsigned i = vals[t];
        if (i >= info[b].n) i = 0;  // (never taken: compaction fills all N rows of a slot with indices < n; a guard against a read past the cloud)
        const long long row = info[b].row0 + (long long)i;
        const float x0 = xyz[3 * row], x1 = xyz[3 * row + 1], x2 = xyz[3 * row + 2];
        float* f = s_f + threadIdx.x * F;
        s_x[3 * threadIdx.x] = x0;
        s_x[3 * threadIdx.x + 1] = x1;
        s_x[3 * threadIdx.x + 2] = x2;
        f[0] = x0;
        f[1] = x1;
        f[2] = x2;
        const float* m = mods + row * C;
        if (C == 4 && (reinterpret_cast<uintptr_t>(mods) & 15) == 0) {
            const float4 v = *reinterpret_cast<const float4*>(m);
            f[3] = v.x; f[4] = v.y; f[5] = v.z; f[6] = v.w;
        } else {
            for (int k = 0; k < C; ++k) f[3 + k] = m[k];
        }
        out_i[t] = (int32_t)i;
        if (out_l) out_l[t] = labels ? labels[row] : 0;
    }
    __syncthreads();
    const bool vec = ((reinterpret_cast<uintptr_t>(out_xyz) | reinterpret_cast<uintptr_t>(out_f)) & 15) == 0;
    store_staged_words(s_x, out_xyz + (size_t)t0 * 3, rows * 3, vec);
    store_staged_words(s_f, out_f + (size_t)t0 * F, rows * F, vec);
}

// positives per cloud: thread = 16 consecutive rows, one atomic per cloud run.  grid over the bank's rows.
__global__ __launch_bounds__(256) void cloud_positive_count_kernel(const int32_t* __restrict__ labels, const long long* __restrict__ off,
                                                                   int n_clouds, long long total, unsigned* __restrict__ counts)
{
    const long long r0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 16;
    if (r0 >= total) return;
    const long long r1 = r0 + 16 < total ? r0 + 16 : total;
    int lo = 0, hi = n_clouds - 1;  // the cloud holding r0: the last c with off[c] <= r0
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= r0) lo = mid;
        else hi = mid - 1;
    }
    int c = lo;
    unsigned cnt = 0;
    for (long long r = r0; r < r1; ++r) {
        while (c + 1 < n_clouds && r >= off[c + 1]) {
            if (cnt) atomicAdd(&counts[c], cnt);
            cnt = 0;
            ++c;
        }
        cnt += labels[r] > 0;
    }
    if (cnt) atomicAdd(&counts[c], cnt);
}

}  // namespace

}  // namespace ps

extern "C" int ps_cloud_positive_counts(ps_context* c, const int32_t* labels, const int64_t* offsets, int64_t n_clouds, int64_t* counts)
{
    using namespace ps;
    PS_CHECK(c && offsets && counts, "ps_cloud_positive_counts: NULL argument");
    PS_CHECK(n_clouds >= 1 && n_clouds < (1ll << 31), "ps_cloud_positive_counts: n_clouds = %lld out of range", (long long)n_clouds);
    PS_CHECK(offsets[0] >= 0, "ps_cloud_positive_counts: offsets[0] = %lld is negative", (long long)offsets[0]);
    for (int64_t k = 0; k < n_clouds; ++k)
        PS_CHECK(offsets[k + 1] >= offsets[k] && offsets[k + 1] - offsets[k] < (1ll << 31),
                 "ps_cloud_positive_counts: cloud %lld has offsets [%lld, %lld)", (long long)k, (long long)offsets[k], (long long)offsets[k + 1]);
    if (!labels) {
        for (int64_t k = 0; k < n_clouds; ++k) counts[k] = 0;
        return PS_OK;
    }
    PS_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const long long row0 = offsets[0], total = offsets[n_clouds] - row0;
    Arena& A = c->sample_arena;
    long long* d_off = nullptr;
    unsigned* d_cnt = nullptr;
    for (int pass = 0; pass < 2; ++pass) {
        A.begin(pass == 0);
        d_off = A.take<long long>(n_clouds + 1);
        d_cnt = A.take<unsigned>(n_clouds);
        if (pass == 0) PS_TRY(A.buf.reserve(A.off));
    }
    std::vector<long long> rel(n_clouds + 1);
    for (int64_t k = 0; k <= n_clouds; ++k) rel[k] = offsets[k] - row0;
    Stage stg(c, "cloud_sample", 1);
    PS_HIP(hipMemcpyAsync(d_off, rel.data(), sizeof(long long) * rel.size(), hipMemcpyHostToDevice, st));
    PS_HIP(hipMemsetAsync(d_cnt, 0, sizeof(unsigned) * n_clouds, st));
    if (total > 0)
        hipLaunchKernelGGL(cloud_positive_count_kernel, dim3((unsigned)((total + 4095) / 4096)), dim3(256), 0, st, labels + row0, d_off, (int)n_clouds,
                           total, d_cnt);
    PS_HIP(hipGetLastError());
    std::vector<unsigned> h(n_clouds);
    PS_HIP(hipMemcpyAsync(h.data(), d_cnt, sizeof(unsigned) * n_clouds, hipMemcpyDeviceToHost, st));
    PS_HIP(hipStreamSynchronize(st));
    for (int64_t k = 0; k < n_clouds; ++k) counts[k] = h[k];
    return PS_OK;
}

extern "C" int ps_cloud_sample(ps_context* c, const float* xyz, const float* modalities, int32_t C, const int32_t* labels, const int64_t* offsets,
                               int64_t n_clouds, const int64_t* positives, const int32_t* cloud_ids, int32_t B, int64_t N, uint32_t seed,
                               float* out_xyz, float* out_features, int32_t* out_labels, int32_t* out_idx)
{
    using namespace ps;
    // every argument error is found here, before anything is enqueued
    PS_CHECK(c && xyz && modalities && offsets && cloud_ids && out_xyz && out_features && out_idx, "ps_cloud_sample: NULL argument");
    PS_CHECK(!labels || positives, "ps_cloud_sample: positives_host is NULL while labels are given");
    PS_CHECK(C >= 1 && C <= PS_CLOUD_SAMPLE_MAX_C, "ps_cloud_sample: C = %d, must be in [1, %d]", (int)C, PS_CLOUD_SAMPLE_MAX_C);
    PS_CHECK(B >= 1 && B <= PS_CLOUD_SAMPLE_MAX_B, "ps_cloud_sample: B = %d, must be in [1, %d]", (int)B, PS_CLOUD_SAMPLE_MAX_B);
    PS_CHECK(N >= 1 && (int64_t)B * N < (1ll << 31), "ps_cloud_sample: N = %lld with B = %d (need N >= 1 and B * N < 2^31)", (long long)N, (int)B);
    PS_CHECK(n_clouds >= 1, "ps_cloud_sample: n_clouds = %lld", (long long)n_clouds);
    std::vector<SlotInfo> info(B);
    unsigned max_n = 0;
    for (int b = 0; b < B; ++b) {
        const int32_t cl = cloud_ids[b];
        PS_CHECK(cl >= 0 && cl < n_clouds, "ps_cloud_sample: cloud_ids[%d] = %d is not a cloud of the bank (%lld clouds)", b, (int)cl, (long long)n_clouds);
        const int64_t r0 = offsets[cl], n = offsets[cl + 1] - offsets[cl];
        PS_CHECK(r0 >= 0 && n >= 0 && n < (1ll << 31), "ps_cloud_sample: cloud %d has offsets [%lld, %lld)", (int)cl, (long long)r0,
                 (long long)offsets[cl + 1]);
        PS_CHECK(N <= n, "ps_cloud_sample: N = %lld is larger than cloud %d (%lld points)", (long long)N, (int)cl, (long long)n);
        const int64_t p = labels ? positives[cl] : 0;
        PS_CHECK(p >= 0 && p <= N, "ps_cloud_sample: cloud %d has %lld positive points, more than N = %lld", (int)cl, (long long)p, (long long)N);
        SlotInfo& s = info[b];
        s.row0 = r0;
        s.n = (unsigned)n;
        s.s_sel = hash32(seed + kSeedMul * (2u * b + 1u));
        s.s_perm = hash32(seed + kSeedMul * (2u * b + 2u));
        s.p_host = (unsigned)p;
        s.cloud = cl;
        s.pad = 0;
        max_n = std::max(max_n, s.n);
    }
    PS_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const size_t total = (size_t)B * (size_t)N;
    const unsigned ntiles = (max_n + kTile - 1) / kTile;
    const size_t sort_words = sort_workspace_words(total);
    Arena& A = c->sample_arena;
    SlotInfo* d_info = nullptr;
    SampleSlot* d_slots = nullptr;
    int* d_status = nullptr;
    unsigned* d_tiles = nullptr;
    unsigned long long *k0 = nullptr, *k1 = nullptr;
    unsigned *v0 = nullptr, *v1 = nullptr, *work = nullptr;
    for (int pass = 0; pass < 2; ++pass) {
        A.begin(pass == 0);
        d_info = A.take<SlotInfo>(B);
        d_slots = A.take<SampleSlot>(B);
        d_status = A.take<int>(4);
        d_tiles = A.take<unsigned>((size_t)2 * B * ntiles);
        k0 = A.take<unsigned long long>(total);
        k1 = A.take<unsigned long long>(total);
        v0 = A.take<unsigned>(total);
        v1 = A.take<unsigned>(total);
        work = A.take<unsigned>(sort_words);
        if (pass == 0) PS_TRY(A.buf.reserve(A.off));
    }
    int bits = 32;  // the slot above the 32-bit permutation hash
    while ((1 << (bits - 32)) < B) ++bits;
    {
        Stage stg(c, "cloud_sample", 1);
        PS_TRY(c->upload_async(d_info, info.data(), sizeof(SlotInfo) * B));
        hipLaunchKernelGGL(cloud_sample_init_kernel, dim3(B), dim3(256), 0, st, d_slots, d_status);
        const dim3 grid(ntiles, B);
        for (int shift = 24; shift >= 0; shift -= 8) {
            hipLaunchKernelGGL(cloud_sample_hist_kernel, grid, dim3(256), 0, st, labels, d_info, d_slots, shift);
            hipLaunchKernelGGL(cloud_sample_pick_kernel, dim3(B), dim3(256), 0, st, d_info, d_slots, d_status, (unsigned)N, shift);
        }
        hipLaunchKernelGGL(cloud_sample_compact_kernel<false>, grid, dim3(256), 0, st, labels, d_info, d_slots, d_tiles, ntiles, (unsigned)N, k0, v0);
        hipLaunchKernelGGL(cloud_sample_tile_scan_kernel, dim3(B), dim3(256), 0, st, d_info, d_tiles, ntiles);
        hipLaunchKernelGGL(cloud_sample_compact_kernel<true>, grid, dim3(256), 0, st, labels, d_info, d_slots, d_tiles, ntiles, (unsigned)N, k0, v0);
        const int which = radix_sort_pairs_u64(st, k0, k1, v0, v1, total, bits, work);
        const unsigned* sorted = which == 0 ? v0 : v1;
        hipLaunchKernelGGL(cloud_sample_gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, xyz, modalities, (int)C, labels, d_info,
                           sorted, (unsigned)N, (unsigned)total, out_xyz, out_features, out_labels, out_idx);
        PS_HIP(hipGetLastError());
        stg.n = 1 + 8 + 3 + radix_sort_pairs_launches(total, bits) + 1;
    }
    // the device's positive counts against positives_host: a stale table is PS_ESTATE (the batch was drawn with the device's counts)
    if (c->deferred) return c->defer_status(d_status, 4 * sizeof(int), 1, c->samples++);
    int32_t h_status[4] = {0, 0, 0, 0};
    PS_HIP(hipMemcpyAsync(h_status, d_status, sizeof h_status, hipMemcpyDeviceToHost, st));
    PS_HIP(hipStreamSynchronize(st));
    ++c->samples;
    if (h_status[0]) {
        ps::set_error("ps_cloud_sample: slot %d (cloud %d) has %d positive labels on the device, positives_host says %d: the table is stale "
                      "(the batch was drawn with the device's count)", h_status[1], (int)cloud_ids[h_status[1]], h_status[2], h_status[3]);
        return PS_ESTATE;
    }
    return PS_OK;
}
