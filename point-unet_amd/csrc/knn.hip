// knn.hip -- exact KNN search kernel + the C-ABI entry points built on it (ps_knn_batch, ps_pyramid_build).
//
// Replaces cpp_knn_batch_omp (PointSegment/utils/nearest_neighbors/knn_.cxx:104-135) and the per-layer loop
// of tf_map (PointSegment/runBraTS.py:147-156).
//
// Kernel shape: one lane per query, the per-query routine of kdtree.h (iterative descent with an explicit
// deferred-node stack, top-K list in registers).  Lanes of a wave are given queries in the *support tree's
// leaf order* whenever the caller can provide it (self-queries and the pyramid's up-sampling queries), so a
// wave walks almost the same root-to-leaf path and its node/leaf loads hit the same cache lines.
// Roofline: neither HBM nor MFMA -- a divergent, latency-bound tree walk; reported in queries/s with the
// algorithmic bytes of SURVEY 8(d) next to it.
#include "common.h"
#include "kdtree.h"
#include "kdtree_build.h"

#include <cfloat>
#include <cstring>

namespace ps {

struct KnnJob {
    TreeView tree;
    const float4* q4;   // queries as (x,y,z,bitcast row) -- e.g. another tree's `pts` -- or NULL
    const float* q3;    // raw [nq,3] queries (row = query position) when q4 == NULL
    int32_t nq;
    int32_t* out;       // [nq, K]
    int32_t* overflow;  // the tree set's status words (BuildFlag): kFlagStackOverflow is set if any query overflowed the deferred-node stack
    int32_t* order;     // optional [nq]: order[t] = row of the t-th query (self queries: the tree's leaf order, for ps_pyramid.order)
    int32_t prefix = 0; // != 0: the tree holds exactly the rows [0, tree.n) of the cloud the q4 queries come from (up-sampling queries)
    int32_t sub_m = 0;  // rows [0, sub_m) are ALSO written to sub_out [sub_m, K]: the pooling table of tf_map, pool = neigh_idx[:, :N // r]
    int32_t* sub_out = nullptr;  // (runBraTS.py:150) -- written by the lane that owns the row, no slice launch behind the search
};

static_assert(sizeof(KnnJob) <= 128, "TreeSetPlan::carve reserves 128 bytes per job");

// Deferred-node stack of the search kernels: the kWin most recent entries of every lane live in LDS
// ([slot][word][thread]: a wave's access to one word is one conflict-free row), older ones spill to per-lane scratch
// and come back only when the window has drained.  A pop is the head of the next dependent node load, so its latency
// (LDS ~100 cycles vs a scratch round trip through L2/HBM) is on the critical path of every query; the first descent
// pushes ~log2(n/10) entries, of which the shallow ones -- spilled -- are almost always pruned by their `m` alone.
#ifndef PS_KNN_WIN
#define PS_KNN_WIN 8
#endif
constexpr int kWin = PS_KNN_WIN;  // (a power of two)
// Threads per search workgroup (the LDS window is [slot][word][thread]).  ONE wave: the kernel has no workgroup-level step, and a
// workgroup retires as soon as its own 64 queries are done instead of with the slowest of four waves -- its LDS and wave slot go to the next
// workgroup (or to another lane's kernel) that much earlier.  Measured (round 4, same box): 256 threads 0.182 ms / pipelined step 0.860,
// 128: 0.172 / 0.850, 64: 0.168 / 0.833, 512: 0.211 / 0.880.
#ifndef PS_KNN_THREADS
#define PS_KNN_THREADS 64
#endif
constexpr int kKnnThreads = PS_KNN_THREADS;
// the spill arrays live in their own object: indexed dynamically, they stay in scratch memory, and as members of WindowStack they
// kept its sp / lo counters there too (a scratch store per push, a scratch load in front of every pop)
struct SpillStore {
    int sid[kStackMax];
    float sm[kStackMax], s0[kStackMax], s1[kStackMax], s2[kStackMax];
};
struct WindowStack {
    typedef __attribute__((address_space(3))) float lds_float;
    lds_float* w;  // LDS base of this thread (already offset by threadIdx.x); word stride = kKnnThreads (one word per thread and slot)
    SpillStore* sp_;  // entries [0, lo)
    int sp = 0, lo = 0;  // entries [lo, sp) are in LDS at slot (depth % kWin); [0, lo) in scratch
    __device__ __forceinline__ bool push(int node, float mm, float a, float b, float c)
    {
        if (sp >= kStackMax) return false;
        if (sp - lo == kWin) {  // spill the oldest windowed entry
            const lds_float* e = w + (lo & (kWin - 1)) * 5 * kKnnThreads;
            sp_->sid[lo] = __float_as_int(e[0]); sp_->sm[lo] = e[kKnnThreads]; sp_->s0[lo] = e[2 * kKnnThreads]; sp_->s1[lo] = e[3 * kKnnThreads]; sp_->s2[lo] = e[4 * kKnnThreads];
            ++lo;
        }
        lds_float* e = w + (sp & (kWin - 1)) * 5 * kKnnThreads;
        e[0] = __int_as_float(node); e[kKnnThreads] = mm; e[2 * kKnnThreads] = a; e[3 * kKnnThreads] = b; e[4 * kKnnThreads] = c;
        ++sp;
        return true;
    }
    __device__ __forceinline__ bool pop(float worst, int& node, float& mm, float& a, float& b, float& c)
    {
        while (sp > 0) {
            --sp;
            if (sp >= lo) {
                const lds_float* e = w + (sp & (kWin - 1)) * 5 * kKnnThreads;
                const float em = e[kKnnThreads];
                if (em <= worst) {
                    node = __float_as_int(e[0]); mm = em; a = e[2 * kKnnThreads]; b = e[3 * kKnnThreads]; c = e[4 * kKnnThreads];
                    return true;
                }
            } else {
                lo = sp;  // the window is empty; this entry comes from scratch
                if (sp_->sm[sp] <= worst) {
                    node = sp_->sid[sp]; mm = sp_->sm[sp]; a = sp_->s0[sp]; b = sp_->s1[sp]; c = sp_->s2[sp];
                    return true;
                }
            }
        }
        return false;
    }
};

template <int K>
__device__ __forceinline__ void knn_body(const KnnJob& job, float* win)
{
    // XCD-aware order: workgroups go to the 8 XCDs round-robin, and queries are in leaf order, so workgroup b takes the
    // (b / 8)-th block of the (b % 8)-th eighth of the queries -- every XCD's L2 then serves one contiguous eighth of the tree's
    // leaves (plus the shared top levels) instead of all of it.
    const int per_xcd = (((job.nq + (int)blockDim.x - 1) / (int)blockDim.x) + 7) >> 3;  // of THIS job's workgroups
    if ((int)(blockIdx.x >> 3) >= per_xcd) return;
    const int bx = (blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
    const int t = bx * blockDim.x + threadIdx.x;
    if (t >= job.nq) return;
    // (degenerate cloud: a builder queue overflowed and the tree has holes.  Unreachable for real clouds -- the queues are sized
    // for the worst disjoint-range count -- but whatever runs behind this kernel without a host check must still find valid
    // indices: the rows are filled with index 0 instead of walking a broken tree; the status word reports the failure.)
    const bool broken = gload(job.overflow + kFlagQueueOverflow) != 0;
    float qx, qy, qz;
    int row;
    if (job.q4) {
        const float4 q = gload(job.q4 + t);
        qx = q.x; qy = q.y; qz = q.z;
        row = broken ? t : as_i(q.w);
        if (job.order) gstore(job.order + t, row);
    } else {
        qx = gload(job.q3 + 3 * (size_t)t);
        qy = gload(job.q3 + 3 * (size_t)t + 1);
        qz = gload(job.q3 + 3 * (size_t)t + 2);
        row = t;
    }
    if (broken) {
        for (int j = 0; j < K; ++j) gstore(job.out + (size_t)row * K + j, 0);
        if (row < job.sub_m)
            for (int j = 0; j < K; ++j) gstore(job.sub_out + (size_t)row * K + j, 0);
        return;
    }
    float dist[K];
    int idx[K];
    // Self-queries (the queries ARE this tree's points, lanes in leaf order): the K points around the query in leaf order are K
    // distinct tree points, so the K-th neighbour distance is at most the largest of their distances m.  The list then starts as K
    // phantom entries at a distance just above m instead of +inf: every true neighbour (d <= m) still enters in visit order and
    // pushes the phantoms out -- the result, ties included, is that of the same search on a tree with K extra far points --
    // but sub-trees beyond m are pruned from the first step and the early fill-the-list insertions disappear.
    float seed = FLT_MAX;
    if (K > 1 && job.q4 == job.tree.pts && job.nq >= K) {
        if constexpr (K <= 32) {
            if (job.nq >= 2 * K - 1) {
                // every K-wide window of the (2K-1)-point span around the query bounds the K-th distance by its largest member: take
                // the tightest.  (Leaf order is only locally spatial: a query next to a high split plane has far points on one side,
                // and in a wave the lane with the loosest bound sets the pace.)  Window [s, s+K) = suffix of the left half from s +
                // prefix of the right half up to s+K-1.
                const int w0 = min(max(t - (K - 1), 0), job.nq - (2 * K - 1));
                float d[2 * K - 1];
#pragma unroll
                for (int j = 0; j < 2 * K - 1; ++j) {
                    const float4 p = gload(job.q4 + w0 + j);
                    d[j] = sq_dist(qx, qy, qz, p.x, p.y, p.z);
                }
#pragma unroll
                for (int j = K - 3; j >= 0; --j) d[j] = fmaxf(d[j], d[j + 1]);          // d[j] = max(d[j .. K-2]), j <= K-2
#pragma unroll
                for (int j = K; j < 2 * K - 1; ++j) d[j] = fmaxf(d[j], d[j - 1]);      // d[j] = max(d[K-1 .. j]), j >= K-1
                float m = d[K - 1 + K - 1];                                            // window s = K-1: the right half alone
#pragma unroll
                for (int sft = 0; sft < K - 1; ++sft) m = fminf(m, fmaxf(d[sft], d[sft + K - 1]));
                seed = __fadd_rn(__fadd_rn(m, __fmul_rn(m, 1e-6f)), 1e-30f);  // strictly above m (m >= 0)
            }
        }
        if (seed == FLT_MAX) {
            const int w0 = min(max(t - K / 2, 0), job.nq - K);
            float m = 0.f;
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const float4 p = gload(job.q4 + w0 + j);
                m = fmaxf(m, sq_dist(qx, qy, qz, p.x, p.y, p.z));
            }
            seed = __fadd_rn(__fadd_rn(m, __fmul_rn(m, 1e-6f)), 1e-30f);
        }
    }
    if (K == 1 && job.prefix && job.q4 != nullptr && job.nq >= 32) {
        // up-sampling query (runBraTS.py:151): the queries are the points of level i in THEIR leaf order, the tree holds the prefix
        // subset xyz[:n] of the same cloud.  A leaf-order neighbour of the query whose row is < n is a point of the searched tree, so
        // its distance bounds the 1-NN distance: start from a phantom just above the smallest such distance among 32 neighbours
        // (same argument as above; a query that is in the subset itself finds distance 0).  Measured: the exact bound taken from the
        // query's finished K-NN list is no faster (0.060 vs 0.057 ms) -- what is left is the descent itself.
        const int w0 = min(max(t - 16, 0), job.nq - 32);
        float m = FLT_MAX;
#pragma unroll
        for (int j = 0; j < 32; ++j) {
            const float4 p = gload(job.q4 + w0 + j);
            const float dd = sq_dist(qx, qy, qz, p.x, p.y, p.z);
            m = as_i(p.w) < job.tree.n ? fminf(m, dd) : m;
        }
        if (m < FLT_MAX) seed = __fadd_rn(__fadd_rn(m, __fmul_rn(m, 1e-6f)), 1e-30f);
    }
#pragma unroll
    for (int j = 0; j < K; ++j) {
        dist[j] = seed;
        idx[j] = 0;
    }
    SpillStore spill;
    WindowStack st;
    st.sp_ = &spill;
    st.w = (WindowStack::lds_float*)(win + threadIdx.x);
    const bool ok = knn_search_one<K, WindowStack>(job.tree, qx, qy, qz, dist, idx, st);
    if (!ok) gstore(job.overflow + kFlagStackOverflow, 1);
    int32_t* o = job.out + (size_t)row * K;
    int32_t* o2 = row < job.sub_m ? job.sub_out + (size_t)row * K : nullptr;
    if constexpr (K % 4 == 0) {
#pragma unroll
        for (int j = 0; j < K; j += 4) gstore(reinterpret_cast<int4*>(o + j), make_int4(idx[j], idx[j + 1], idx[j + 2], idx[j + 3]));
        if (o2) {
#pragma unroll
            for (int j = 0; j < K; j += 4) gstore(reinterpret_cast<int4*>(o2 + j), make_int4(idx[j], idx[j + 1], idx[j + 2], idx[j + 3]));
        }
    } else {
#pragma unroll
        for (int j = 0; j < K; ++j) gstore(o + j, idx[j]);
        if (o2) {
#pragma unroll
            for (int j = 0; j < K; ++j) gstore(o2 + j, idx[j]);
        }
    }
}

// (experiment knob: -DPS_KNN_WAVES_PER_EU=n makes the register allocator fit n waves per SIMD)
#ifdef PS_KNN_WAVES_PER_EU
#define PS_KNN_OCC __attribute__((amdgpu_waves_per_eu(PS_KNN_WAVES_PER_EU, PS_KNN_WAVES_PER_EU)))
#else
#define PS_KNN_OCC
#endif

template <int K>
__global__ __launch_bounds__(kKnnThreads) PS_KNN_OCC void knn_kernel(const KnnJob* __restrict__ jobs)
{
    __shared__ float win[kWin * 5 * kKnnThreads];
    knn_body<K>(jobs[blockIdx.y], win);
}

// The pyramid's two searches in ONE launch: jobs [0, n_first) are the K-NN self queries, the rest the 1-NN up-sampling queries.  The
// K-NN search ends with a long tail (its duration is its slowest wave's; the chip holds all of its waves at once), and a second launch
// cannot start under it: here the 1-NN workgroups are dispatched as the K-NN ones retire.
template <int K>
__global__ __launch_bounds__(kKnnThreads) PS_KNN_OCC void knn_pair_kernel(const KnnJob* __restrict__ jobs, int n_first)
{
    __shared__ float win[kWin * 5 * kKnnThreads];
    if ((int)blockIdx.y < n_first) knn_body<K>(jobs[blockIdx.y], win);
    else knn_body<1>(jobs[blockIdx.y], win);
}

__global__ void widen_kernel(const int32_t* __restrict__ in, int64_t* __restrict__ out, size_t count)
{
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i < count) out[i] = in[i];
}

// One workgroup per kKnnThreads queries of the largest job, rounded up to a multiple of 8: the XCD remap in knn_body covers [0, grid.x) exactly.
static dim3 knn_grid(int max_nq, int n_jobs) { return dim3((ceil_div(max_nq, kKnnThreads) + 7) & ~7, n_jobs); }

// (the compiled K: PS_KNN_KS / PS_KNN_PAIR_KS of kdtree.h -- the pair kernel has every size but K = 1)
static int launch_knn(ps_context* c, const KnnJob* d_jobs, int n_jobs, int max_nq, int K)
{
    const dim3 grid = knn_grid(max_nq, n_jobs);
    if (grid.x == 0 || n_jobs == 0) return PS_OK;
    switch (K) {
#define PS_KCASE(k) case k: hipLaunchKernelGGL(knn_kernel<k>, grid, dim3(kKnnThreads), 0, c->stream, d_jobs); break;
        PS_KNN_KS(PS_KCASE)
#undef PS_KCASE
        default:
            set_error("ps_knn: K=%d is not a compiled size (" PS_KNN_KS_TEXT ")", K);
            return PS_EINVAL;
    }
    PS_HIP(hipGetLastError());
    return PS_OK;
}

static int launch_knn_pair(ps_context* c, const KnnJob* d_jobs, int n_first, int n_jobs, int max_nq, int K)
{
    if (K == 1) return launch_knn(c, d_jobs, n_jobs, max_nq, 1);
    const dim3 grid = knn_grid(max_nq, n_jobs);
    if (grid.x == 0 || n_jobs == 0) return PS_OK;
    switch (K) {
#define PS_KCASE(k) case k: hipLaunchKernelGGL(knn_pair_kernel<k>, grid, dim3(kKnnThreads), 0, c->stream, d_jobs, n_first); break;
        PS_KNN_PAIR_KS(PS_KCASE)
#undef PS_KCASE
        default:
            set_error("ps_pyramid_build: K=%d is not a compiled size (" PS_KNN_KS_TEXT ")", K);
            return PS_EINVAL;
    }
    PS_HIP(hipGetLastError());
    return PS_OK;
}
}  // namespace ps

using namespace ps;

// --------------------------------------------------------------------------------------------------------
// ps_knn_batch
// --------------------------------------------------------------------------------------------------------
static int knn_batch_impl(ps_context* c, const float* support, const float* queries, int64_t B, int64_t n1, int64_t n2,
                          int64_t dim, int64_t K, int32_t* out32, int64_t* out64, int device_ptrs)
{
    PS_CHECK(c != nullptr, "ps_knn_batch: ctx is NULL");
    PS_CHECK(dim == 3, "ps_knn_batch: dim must be 3 (got %lld)", (long long)dim);
    PS_CHECK(B >= 0 && n1 >= 0 && n2 >= 0, "ps_knn_batch: negative size");
    PS_CHECK(n1 < kMaxTreePoints, "ps_knn_batch: n_support too large (limit 2^25 points per cloud)");
    PS_CHECK(out32 != nullptr || out64 != nullptr, "ps_knn_batch: out_idx is NULL");
    // (K < 1 included; refused here, before anything is staged or built: launch_knn's own refusal would come behind the copies and the
    // tree build)
    PS_CHECK(knn_k_compiled(K), "ps_knn: K=%lld is not a compiled size (" PS_KNN_KS_TEXT ")", (long long)K);
    if (B == 0 || n2 == 0) return PS_OK;
    PS_CHECK(support != nullptr || n1 == 0, "ps_knn_batch: support is NULL");
    PS_CHECK(queries != nullptr, "ps_knn_batch: queries is NULL");
    PS_HIP(hipSetDevice(c->device));

    const size_t out_count = (size_t)B * n2 * K;
    const float* d_support = support;
    const float* d_queries = queries;
    int32_t* d_out32 = out32;
    int64_t* d_out64 = out64;
    if (!device_ptrs) {
        const size_t sb = (size_t)B * n1 * 3 * sizeof(float), qb = (size_t)B * n2 * 3 * sizeof(float);
        PS_TRY(c->stage_in.reserve(sb + qb + 512));
        PS_TRY(c->stage_out.reserve(out_count * (out64 ? 12 : 4) + 512));
        float* ds = c->stage_in.as<float>();
        float* dq = reinterpret_cast<float*>(c->stage_in.as<char>() + ((sb + 255) & ~size_t(255)));
        if (sb) PS_HIP(hipMemcpyAsync(ds, support, sb, hipMemcpyHostToDevice, c->stream));
        PS_HIP(hipMemcpyAsync(dq, queries, qb, hipMemcpyHostToDevice, c->stream));
        d_support = ds;
        d_queries = dq;
        d_out32 = c->stage_out.as<int32_t>();
        d_out64 = out64 ? reinterpret_cast<int64_t*>(c->stage_out.as<char>() + ((out_count * 4 + 255) & ~size_t(255))) : nullptr;
    } else if (out64) {
        // device int64 output: search into a scratch int32 image first
        PS_TRY(c->stage_out.reserve(out_count * 4 + 256));
        d_out32 = c->stage_out.as<int32_t>();
    }

    // plan + carve the workspace: B trees and the job table
    TreeSetPlan plan;
    for (int64_t b = 0; b < B; ++b) plan.add((int32_t)n1);
    for (int pass = 0; pass < 2; ++pass) {
        c->knn_arena.begin(pass == 0);
        plan.carve(c->knn_arena);
        if (pass == 0) PS_TRY(c->knn_arena.buf.reserve(c->knn_arena.off));
    }
    std::vector<KnnJob> jobs(B);
    for (int64_t b = 0; b < B; ++b) {
        jobs[b].tree = plan.view((int)b);
        jobs[b].q4 = nullptr;
        jobs[b].q3 = d_queries + (size_t)b * n2 * 3;
        jobs[b].nq = (int32_t)n2;
        jobs[b].out = d_out32 + (size_t)b * n2 * K;
        jobs[b].overflow = plan.d_flags;
        jobs[b].order = nullptr;
    }
    std::memcpy(plan.host_jobs(), jobs.data(), sizeof(KnnJob) * B);  // (travels with the builder's own tables: one copy, kdtree_build.h)
    {
        Stage st(c, "kdtree_build", 1);
        for (int64_t b = 0; b < B; ++b) plan.src[b] = d_support + (size_t)b * n1 * 3;
        PS_TRY(build_trees(c, plan));
    }
    int32_t flag[kBuildFlagWords] = {};
    {
        Stage st(c, "knn_search", 1);
        PS_TRY(launch_knn(c, reinterpret_cast<const KnnJob*>(plan.d_jobs), (int)B, (int)n2, (int)K));
    }
    if (out64) {
        hipLaunchKernelGGL(widen_kernel, dim3(ceil_div(out_count, 256)), dim3(256), 0, c->stream, d_out32, d_out64 ? d_out64 : out64,
                           out_count);
        PS_HIP(hipGetLastError());
    }
    if (!device_ptrs) {
        if (out64)
            PS_HIP(hipMemcpyAsync(out64, d_out64, out_count * 8, hipMemcpyDeviceToHost, c->stream));
        else
            PS_HIP(hipMemcpyAsync(out32, d_out32, out_count * 4, hipMemcpyDeviceToHost, c->stream));
    }
    PS_HIP(hipMemcpyAsync(flag, plan.d_flags, sizeof(flag), hipMemcpyDeviceToHost, c->stream));
    // (the job table and the plan's staging live in host memory of this frame: wait before returning)
    PS_HIP(hipStreamSynchronize(c->stream));
    PS_CHECK(flag[kFlagQueueOverflow] == 0, "ps_knn_batch: kd-tree builder queue overflow (degenerate cloud)");
    PS_CHECK(flag[kFlagStackOverflow] == 0, "ps_knn_batch: kd-tree deeper than the %d-entry traversal stack", kStackMax);
    return PS_OK;
}

extern "C" int ps_knn_batch(ps_context* c, const float* support, const float* queries, int64_t B, int64_t n1, int64_t n2,
                            int64_t dim, int64_t K, int32_t* out_idx, int device_ptrs)
{
    return knn_batch_impl(c, support, queries, B, n1, n2, dim, K, out_idx, nullptr, device_ptrs);
}

extern "C" int ps_knn_batch_i64(ps_context* c, const float* support, const float* queries, int64_t B, int64_t n1, int64_t n2,
                                int64_t dim, int64_t K, int64_t* out_idx, int device_ptrs)
{
    return knn_batch_impl(c, support, queries, B, n1, n2, dim, K, nullptr, out_idx, device_ptrs);
}

// --------------------------------------------------------------------------------------------------------
// ps_pyramid_build
// --------------------------------------------------------------------------------------------------------
namespace ps {

}  // namespace ps

extern "C" int ps_pyramid_build(ps_context* c, const float* xyz0, int64_t B, int64_t n0, int32_t L, const int32_t* ratios, int32_t K,
                                ps_pyramid* pyr)
{
    PS_CHECK(c && xyz0 && ratios && pyr, "ps_pyramid_build: NULL argument");
    PS_CHECK(L >= 1 && L <= PS_MAX_LAYERS, "ps_pyramid_build: num_layers %d out of range", L);
    PS_CHECK(B >= 1 && n0 >= 1 && n0 < kMaxTreePoints, "ps_pyramid_build: bad B / n0");
    PS_HIP(hipSetDevice(c->device));
    int64_t n[PS_MAX_LAYERS + 1];
    n[0] = n0;
    for (int i = 0; i < L; ++i) {
        PS_CHECK(ratios[i] >= 1, "ps_pyramid_build: ratio[%d] < 1", i);
        n[i + 1] = n[i] / ratios[i];
        PS_CHECK(n[i + 1] >= 1, "ps_pyramid_build: level %d would be empty", i + 1);
    }
    pyr->built = 0;
    // (refused here, before the trees are built and xyz[] is written: launch_knn_pair's own refusal would come behind all of that)
    PS_CHECK(knn_k_compiled(K), "ps_pyramid_build: K=%d is not a compiled size (" PS_KNN_KS_TEXT ")", (int)K);
    pyr->num_layers = L;
    pyr->K = K;
    pyr->B = B;
    for (int i = 0; i <= L; ++i) pyr->n[i] = n[i];
    for (int i = 0; i < L; ++i)
        PS_CHECK(pyr->xyz[i] && pyr->neigh_idx[i] && pyr->sub_idx[i] && pyr->interp_idx[i], "ps_pyramid_build: NULL buffer at layer %d", i);

    // trees: (level l in 0..L) x (cloud b).  Level l's point set is the first n[l] points of every cloud.
    TreeSetPlan plan;
    for (int l = 0; l <= L; ++l)
        for (int64_t b = 0; b < B; ++b) plan.add((int32_t)n[l]);
    plan.extra_jobs = (int)(2 * L * B);
    for (int pass = 0; pass < 2; ++pass) {
        c->knn_arena.begin(pass == 0);
        plan.carve(c->knn_arena);
        if (pass == 0) PS_TRY(c->knn_arena.buf.reserve(c->knn_arena.off));
    }
    // every tree reads its prefix of the caller's cloud; the builders' first pass also writes those rows to ps_pyramid.xyz[level]
    // (xyz[i] = xyz[:, :n_i], runBraTS.py:149; xyz[0] may be the caller's own buffer) -- no slice launch
    plan.copy_dst.assign((size_t)(L + 1) * B, nullptr);
    for (int l = 0; l <= L; ++l)
        for (int64_t b = 0; b < B; ++b) {
            plan.src[l * B + b] = xyz0 + (size_t)b * n0 * 3;
            if (l < L && !(l == 0 && pyr->xyz[0] == xyz0)) plan.copy_dst[l * B + b] = pyr->xyz[l] + (size_t)b * n[l] * 3;
        }

    // jobs: K-NN self queries per level, then 1-NN up-sampling queries per level, both in the query set's own
    // tree (leaf) order so neighbouring lanes walk neighbouring paths.
    std::vector<KnnJob> jobs;
    jobs.reserve(2 * L * B);
    int max_nq = 0;
    for (int l = 0; l < L; ++l)
        for (int64_t b = 0; b < B; ++b) {
            KnnJob j;
            j.tree = plan.view((int)(l * B + b));
            j.q4 = j.tree.pts;
            j.q3 = nullptr;
            j.nq = (int32_t)n[l];
            j.out = pyr->neigh_idx[l] + (size_t)b * n[l] * K;
            j.overflow = plan.d_flags;
            j.order = pyr->order[l] ? pyr->order[l] + (size_t)b * n[l] : nullptr;
            j.sub_m = (int32_t)n[l + 1];
            j.sub_out = pyr->sub_idx[l] + (size_t)b * n[l + 1] * K;
            jobs.push_back(j);
            max_nq = std::max(max_nq, j.nq);
        }
    const size_t n_self = jobs.size();
    for (int l = 0; l < L; ++l)
        for (int64_t b = 0; b < B; ++b) {
            KnnJob j;
            j.tree = plan.view((int)((l + 1) * B + b));
            j.q4 = plan.view((int)(l * B + b)).pts;
            j.q3 = nullptr;
            j.nq = (int32_t)n[l];
            j.out = pyr->interp_idx[l] + (size_t)b * n[l];
            j.overflow = plan.d_flags;
            j.order = nullptr;
            j.prefix = 1;
            jobs.push_back(j);
        }
    std::memcpy(plan.host_jobs(), jobs.data(), sizeof(KnnJob) * jobs.size());  // (uploaded by build_trees with its own tables: one copy)
    {
        Stage st(c, "kdtree_build", 1);
        PS_TRY(build_trees(c, plan));
        st.n = plan.launches;
    }
    const KnnJob* dj = reinterpret_cast<const KnnJob*>(plan.d_jobs);
    int32_t flag[kBuildFlagWords] = {};
    {
        {
            Stage st(c, "knn_search", 1);  // K-NN self queries and 1-NN up-sampling queries of every level, one launch
            PS_TRY(launch_knn_pair(c, dj, (int)n_self, (int)jobs.size(), max_nq, (int)K));
        }
        if (c->deferred) {
            // no host synchronisation: the status words go to a pinned slot that ps_synchronize() validates; the host
            // tables behind the asynchronous uploads move into the context's ring so they outlive this frame
            PS_TRY(c->defer_status(plan.d_flags, sizeof(int32_t) * kBuildFlagWords, 0, c->builds));
            ++c->builds;
            pyr->built = pyramid_stamp(pyr);
            return PS_OK;  // (all host tables went through the context's pinned upload ring)
        }
        PS_HIP(hipMemcpyAsync(flag, plan.d_flags, sizeof(flag), hipMemcpyDeviceToHost, c->stream));
        PS_HIP(hipStreamSynchronize(c->stream));
    }
    ++c->builds;
    PS_CHECK(flag[kFlagQueueOverflow] == 0, "ps_pyramid_build: kd-tree builder queue overflow (degenerate cloud)");
    PS_CHECK(flag[kFlagStackOverflow] == 0, "ps_pyramid_build: kd-tree deeper than the %d-entry traversal stack", kStackMax);
    pyr->built = pyramid_stamp(pyr);
    return PS_OK;
}
