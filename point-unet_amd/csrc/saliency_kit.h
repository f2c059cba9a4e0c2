// saliency_kit.h -- what saliency.hip (the forward) and saliency_train.hip (the ops with their gradients) share: the vector and logit-row
// accessors, ONE slab-sum frame for every per-(sample, channel) sum over the voxels, the instance norm's moments, the channel attention's
// dense part, the spatial gate, and the range check of a [B, V, C] tensor.
//
// Every sum over voxels is a float64 partial per (slab of 4096 voxels, sample, channel), the threads of a slab added in a fixed order, the
// slabs by reduce_partials.h: no float atomic, two runs give the same bytes, and E[x^2] - E[x]^2 keeps 53 bits.
#pragma once
#include <cstdint>

#include "reduce_partials.h"
#include "scratch.h"

namespace ps {

constexpr int kSlab = 4096;  // voxels per workgroup of a reduction pass
constexpr int kMaxClasses = 16;

// ---- VEC channels of a lane: 16 bytes where C % 4 == 0 and the tensors are 16-byte aligned, a float elsewhere -- the same values either way ------

template <int VEC>
struct Vec;
template <>
struct Vec<1> {
    float v[1];
};
template <>
struct alignas(16) Vec<4> {
    float v[4];
};

template <int VEC>
__device__ __forceinline__ Vec<VEC> vload(const float* p)
{
    return *reinterpret_cast<const Vec<VEC>*>(p);
}

template <int VEC>
__device__ __forceinline__ void vstore(float* p, const Vec<VEC>& a)
{
    *reinterpret_cast<Vec<VEC>*>(p) = a;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the power of two >= min(groups, 1 << max_shift), as a shift: the lanes a row of `groups` lane-sized pieces gets
inline int lane_shift(int groups, int max_shift)
{
    int s = 0;
    while ((1 << s) < groups && s < max_shift) ++s;
    return s;
}

// ---- the slab-sum frame ------------------------------------------------------------------------------------------------------------------------

// tot[b][c][n] = sum over the voxels v of sample b of the n-th of the NS contributions of element (b, v, c).  F: the contributions --
// f(bc, e, d) fills d[k * NS + n] for the VEC channels k from bc = b * C + c on, at element offset e = (b * V + v) * ld + c -- and
// F::kUnroll, how many rows of a thread are in flight at once (the order of the additions does not depend on it).
// grid (slabs, B, lane tiles).  A row of the workgroup is cw = 1 << cshift lanes of VEC channels each; thread t adds the rows t / cw,
// t / cw + 256 / cw, ... of its slab, then the first cw threads add the 256 / cw row sums of their channels, ascending.  part [slab][B][C][NS].
template <int VEC, int NS, class F>
__global__ __launch_bounds__(256) void slab_sum_kernel(F f, int ld, int V, int C, int cshift, double* __restrict__ part)
{
    constexpr int N = VEC * NS;
    __shared__ double ss[N][256];
    const int t = threadIdx.x, cw = 1 << cshift;
    const int c = (blockIdx.z * cw + (t & (cw - 1))) * VEC, rl = t >> cshift, nrl = 256 >> cshift;
    const int b = blockIdx.y, v0 = blockIdx.x * kSlab, v1 = min(V, v0 + kSlab);
    double s[N];
#pragma unroll
    for (int k = 0; k < N; ++k) s[k] = 0.0;
    if (c < C) {
        const size_t base = (size_t)b * V * ld + c;
#pragma unroll F::kUnroll
        for (int v = v0 + rl; v < v1; v += nrl) {
            double d[N];
            f(b * C + c, base + (size_t)v * ld, d);
#pragma unroll
            for (int k = 0; k < N; ++k) s[k] += d[k];
        }
    }
#pragma unroll
    for (int k = 0; k < N; ++k) ss[k][t] = s[k];
    __syncthreads();
    if (t < cw && c < C) {
        double* o = part + (((size_t)blockIdx.x * gridDim.y + b) * C + c) * NS;
#pragma unroll
        for (int k = 0; k < N; ++k) {
            double S = 0.0;
            for (int j = 0; j < nrl; ++j) S += ss[k][j * cw + t];
            o[k] = S;
        }
    }
}

// part [slabs][B][C][NS] -> tot [B][C][NS].  64 lanes of 4 bytes or 8 lanes of 16 (a 128-byte line) per row of the workgroup.
template <int VEC, int NS, class F>
void slab_sum_run(hipStream_t sm, const F& f, int ld, int B, int V, int C, double* part, double* tot)
{
    const int slabs = ceil_div(V, kSlab), nv = B * C * NS, groups = C / VEC, cshift = lane_shift(groups, VEC == 4 ? 3 : 6);
    const dim3 grid((unsigned)slabs, (unsigned)B, (unsigned)ceil_div(groups, 1 << cshift));
    hipLaunchKernelGGL((slab_sum_kernel<VEC, NS, F>), grid, dim3(256), 0, sm, f, ld, V, C, cshift, part);
    hipLaunchKernelGGL(reduce_partials_kernel<double>, dim3((unsigned)ceil_div(nv, 16)), dim3(256), 0, sm, part, slabs, nv, tot);
}

// (x, x^2): the instance norm's statistics
struct SumSquares {
    static constexpr int kUnroll = 4;
    const float* __restrict__ x;
    __device__ __forceinline__ void operator()(int, size_t e, double (&d)[2]) const
    {
        const double f = (double)x[e];
        d[0] = f;
        d[1] = f * f;
    }
};

// tot [B][C][2] = (sum x, sum x^2) of x [B, V, C] at channel pitch ldx
inline void stats_run(hipStream_t sm, const float* x, int ldx, int B, int V, int C, double* part, double* tot)
{
    slab_sum_run<1, 2>(sm, SumSquares{x}, ldx, B, V, C, part, tot);
}

// a [* m]: the channel attention's mean and the gradient of its scale.  With two tensors two rows are four loads in flight; at four rows the
// compiler waits for each tensor's load in turn, which is slower (DESIGN.md 4.11 has the times).
template <int VEC, bool MUL>
struct ColumnSum {
    static constexpr int kUnroll = MUL ? 2 : 4;
    const float* __restrict__ a;
    const float* __restrict__ m;
    __device__ __forceinline__ void operator()(int, size_t e, double (&d)[VEC]) const
    {
        const Vec<VEC> f = vload<VEC>(a + e);
        if (MUL) {
            const Vec<VEC> g = vload<VEC>(m + e);
#pragma unroll
            for (int k = 0; k < VEC; ++k) d[k] = (double)f.v[k] * (double)g.v[k];
        } else {
#pragma unroll
            for (int k = 0; k < VEC; ++k) d[k] = (double)f.v[k];
        }
    }
};

// ---- instance norm ---------------------------------------------------------------------------------------------------------------------------------

// tot[2 i + {0, 1}] = (sum x, sum x^2) over V voxels -> the mean and sqrt(var + eps), the biased variance of tf.nn.moments clamped at 0.
// (The forward divides gamma by the root, the gradient takes its reciprocal: two roundings, so the root is what they share.)
__device__ __forceinline__ double2 moments(const double* __restrict__ tot, int i, int V, float eps)
{
    const double mean = tot[2 * i] / V;
    double var = tot[2 * i + 1] / V - mean * mean;
    var = var > 0.0 ? var : 0.0;
    return make_double2(mean, sqrt(var + (double)eps));
}

// ---- channel attention ---------------------------------------------------------------------------------------------------------------------------

// ChannelWiseAttention3D's dense part (attention.py:166-174) for one sample, by one workgroup of 256: mean[c] = tot[c * stride] / V,
// h = ReLU(mean w1 + b1) (Ch values), s = sigmoid(h w2 + b2), into the caller's LDS arrays; float64 accumulators, ascending.  Ends
// behind a barrier: every thread may read all three.
__device__ __forceinline__ void ca_dense(const double* __restrict__ tot, int stride, int V, int C, int Ch, const float* __restrict__ w1,
                                         const float* __restrict__ b1, const float* __restrict__ w2, const float* __restrict__ b2, float* mean, float* h,
                                         float* s)
{
    const int t = threadIdx.x;
    for (int c = t; c < C; c += 256) mean[c] = (float)(tot[(size_t)c * stride] / V);
    __syncthreads();
    for (int i = t; i < Ch; i += 256) {
        double acc = (double)b1[i];
        for (int c = 0; c < C; ++c) acc += (double)mean[c] * (double)w1[(size_t)c * Ch + i];
        h[i] = fmaxf((float)acc, 0.f);
    }
    __syncthreads();
    for (int c = t; c < C; c += 256) {
        double acc = (double)b2[c];
        for (int i = 0; i < Ch; ++i) acc += (double)h[i] * (double)w2[(size_t)i * C + c];
        s[c] = (float)(1.0 / (1.0 + exp(-acc)));
    }
    __syncthreads();
}

// ---- spatial gate --------------------------------------------------------------------------------------------------------------------------------

// SpatialAttention3D's tail (attention.py:148-152) and model.py:295: sa = sigmoid(a1 + a2 + a3), y = f * sa over the C channels of f
// (pitch ldf) and y (pitch ldy).  grid (ceil(V * C / VEC / 256), B), one lane per (voxel, VEC channels); every lane of a voxel computes
// the voxel's sigmoid and reads its own f before it writes y: y may be f.  V * ldf and V * ldy stay below 2^31 (the callers' limits), so
// only the sample's origin is a 64-bit product, and that one is scalar.
template <int VEC>
__global__ __launch_bounds__(256) void gate_kernel(const float* __restrict__ a1, const float* __restrict__ a2, const float* __restrict__ a3, const float* f,
                                                   int ldf, int V, int C, float* __restrict__ sa, float* y, int ldy)
{
    const unsigned e = blockIdx.x * 256u + threadIdx.x, groups = (unsigned)C / VEC;
    const unsigned v = e / groups, cg = e - v * groups;
    if (v >= (unsigned)V) return;
    const size_t s0 = (size_t)blockIdx.y * V;
    const float z = (a1[s0 + v] + a2[s0 + v]) + a3[s0 + v];
    const float g = 1.f / (1.f + expf(-z));
    if (cg == 0) sa[s0 + v] = g;
    const Vec<VEC> in = vload<VEC>(f + s0 * ldf + (v * (unsigned)ldf + cg * VEC));
    Vec<VEC> o;
#pragma unroll
    for (int k = 0; k < VEC; ++k) o.v[k] = in.v[k] * g;
    vstore<VEC>(y + s0 * ldy + (v * (unsigned)ldy + cg * VEC), o);
}

inline int gate_run(hipStream_t sm, const float* a1, const float* a2, const float* a3, const float* f, int ldf, int B, int V, int C, float* sa, float* y,
                    int ldy)
{
    PS_CHECK((int64_t)V * ldf < (1ll << 31) && (int64_t)V * ldy < (1ll << 31), "gate_run: V = %d times the pitch %d / %d must stay below 2^31", V, ldf, ldy);
    const bool vec = C % 4 == 0 && ldf % 4 == 0 && ldy % 4 == 0 && aligned16(f) && aligned16(y);
    const dim3 grid(blocks256((size_t)V * C / (vec ? 4 : 1)), (unsigned)B);
    if (vec) hipLaunchKernelGGL(gate_kernel<4>, grid, dim3(256), 0, sm, a1, a2, a3, f, ldf, V, C, sa, y, ldy);
    else hipLaunchKernelGGL(gate_kernel<1>, grid, dim3(256), 0, sm, a1, a2, a3, f, ldf, V, C, sa, y, ldy);
    return PS_OK;
}

// ---- a voxel's C logits in registers -------------------------------------------------------------------------------------------------------------

// How they are moved.  MODE 2: C == 2, one 8-byte access; MODE 4: C % 4 == 0, 16-byte accesses; MODE 1: floats.
template <int MODE>
struct Row {
    static constexpr int NC = MODE == 2 ? 2 : kMaxClasses;
    float v[NC];
};

template <int MODE>
__device__ __forceinline__ void row_load(const float* p, int C, Row<MODE>& r)
{
    if (MODE == 2) {
        const float2 a = *reinterpret_cast<const float2*>(p);
        r.v[0] = a.x, r.v[1] = a.y;
    } else if (MODE == 4) {
#pragma unroll
        for (int q = 0; q < Row<MODE>::NC / 4; ++q)
            if (q * 4 < C) {
                const float4 a = *reinterpret_cast<const float4*>(p + q * 4);
                r.v[q * 4] = a.x, r.v[q * 4 + 1] = a.y, r.v[q * 4 + 2] = a.z, r.v[q * 4 + 3] = a.w;
            }
    } else {
#pragma unroll
        for (int c = 0; c < Row<MODE>::NC; ++c)
            if (c < C) r.v[c] = p[c];
    }
}

template <int MODE>
__device__ __forceinline__ void row_store(float* p, int C, const Row<MODE>& r)
{
    if (MODE == 2) {
        *reinterpret_cast<float2*>(p) = make_float2(r.v[0], r.v[1]);
    } else if (MODE == 4) {
#pragma unroll
        for (int q = 0; q < Row<MODE>::NC / 4; ++q)
            if (q * 4 < C) *reinterpret_cast<float4*>(p + q * 4) = make_float4(r.v[q * 4], r.v[q * 4 + 1], r.v[q * 4 + 2], r.v[q * 4 + 3]);
    } else {
#pragma unroll
        for (int c = 0; c < Row<MODE>::NC; ++c)
            if (c < C) p[c] = r.v[c];
    }
}

// softmax in place: the maximum, exp(v - max) and their sum ascending, one division each
template <int MODE>
__device__ __forceinline__ void row_softmax(int C, Row<MODE>& r)
{
    float m = -INFINITY;
#pragma unroll
    for (int c = 0; c < Row<MODE>::NC; ++c)
        if (c < C) m = fmaxf(m, r.v[c]);
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < Row<MODE>::NC; ++c)
        if (c < C) {
            r.v[c] = expf(r.v[c] - m);
            s += r.v[c];
        }
#pragma unroll
    for (int c = 0; c < Row<MODE>::NC; ++c)
        if (c < C) r.v[c] = r.v[c] / s;
}

// the MODE for rows of C floats read at a and written at b
inline int dice_mode(int C, const void* a, const void* b)
{
    if (C == 2 && (reinterpret_cast<uintptr_t>(a) & 7) == 0 && (reinterpret_cast<uintptr_t>(b) & 7) == 0) return 2;
    if (C % 4 == 0 && aligned16(a) && aligned16(b)) return 4;
    return 1;
}

// ---- the range check of a [B, V, C] tensor -------------------------------------------------------------------------------------------------------

enum RowsLimit { kLimitV, kLimitVC, kLimitBVC };  // what has to stay below 2^31: V, V * C or B * V * C

inline int rows_shape_ok(const char* who, int64_t B, int64_t V, int64_t C, int64_t min_C, int64_t max_C, RowsLimit limit)
{
    PS_CHECK(B >= 1 && B <= 65535, "%s: B = %lld, must be in [1, 65535]", who, (long long)B);
    PS_CHECK(C >= min_C && C <= max_C, "%s: C = %lld, must be in [%lld, %lld]", who, (long long)C, (long long)min_C, (long long)max_C);
    const int64_t per_v = limit == kLimitV ? 1 : limit == kLimitVC ? C : B * C;
    PS_CHECK(V >= 1 && V < (1ll << 31) && V * per_v < (1ll << 31), "%s: V = %lld (V >= 1, V%s < 2^31)", who, (long long)V,
             limit == kLimitV ? "" : limit == kLimitVC ? " * C" : " * B * C");
    return PS_OK;
}

}  // namespace ps
