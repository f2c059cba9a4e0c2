// saliency_train.hip -- the channel attention, the spatial gate and softmax + weighted Dice of the saliency attention network, each with its
// gradient (include/pointseg_saliency_attention.h).  Beside conv3d_train.hip these are the ops a training step of
// unet3d_attention still lacked; saliency.hip's forward keeps its own fused forms of the first two and is not touched.
//
// All of them are memory-bound: a pass reads or writes each large tensor once, 16 bytes per lane along the channel axis where C % 4 == 0
// and the tensors are 16-byte aligned (VEC = 4), a float at a time elsewhere (VEC = 1) -- the same values either way, a lane adds its own
// channels only.  Every sum over voxels is a float64 partial per (slab of 4096 voxels, sample), the threads of a slab added in a fixed
// order, the slabs by reduce_partials.h: no float atomic, two runs give the same bytes.
#include <cstdint>

#include "../../include/pointseg_saliency_attention.h"
#include "reduce_partials.h"
#include "scratch.h"

namespace ps {

namespace {

constexpr int kSlab = 4096;  // voxels per workgroup of a reduction pass
constexpr int kMaxC = 1024, kMaxCh = 256, kMaxClasses = 16;

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

// ---- sum over the voxels of a [* m], per (slab, sample, channel) -------------------------------------------------------------------------------

// grid (slabs, B, lane tiles).  A row of the workgroup is cw = 1 << cshift lanes of VEC channels each; thread t adds the rows t / cw,
// t / cw + 256 / cw, ... of its slab, then the first cw threads add the 256 / cw row sums of their channels, ascending.
template <int VEC, bool MUL>
__global__ __launch_bounds__(256) void colsum_kernel(const float* __restrict__ a, const float* __restrict__ m, int V, int C, int cshift, double* __restrict__ part)
{
    __shared__ double ss[VEC][256];
    const int t = threadIdx.x, cw = 1 << cshift;
    const int c = (blockIdx.z * cw + (t & (cw - 1))) * VEC, rl = t >> cshift, nrl = 256 >> cshift;
    const int b = blockIdx.y, v0 = blockIdx.x * kSlab, v1 = min(V, v0 + kSlab);
    double s[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) s[k] = 0.0;
    if (c < C) {
        const size_t base = (size_t)b * V * C + c;
#pragma unroll 4
        for (int v = v0 + rl; v < v1; v += nrl) {
            const Vec<VEC> f = vload<VEC>(a + base + (size_t)v * C);
            if (MUL) {
                const Vec<VEC> g = vload<VEC>(m + base + (size_t)v * C);
#pragma unroll
                for (int k = 0; k < VEC; ++k) s[k] += (double)f.v[k] * (double)g.v[k];
            } else {
#pragma unroll
                for (int k = 0; k < VEC; ++k) s[k] += (double)f.v[k];
            }
        }
    }
#pragma unroll
    for (int k = 0; k < VEC; ++k) ss[k][t] = s[k];
    __syncthreads();
    if (t < cw && c < C) {
        double* o = part + ((size_t)blockIdx.x * gridDim.y + b) * C + c;
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            double S = 0.0;
            for (int j = 0; j < nrl; ++j) S += ss[k][j * cw + t];
            o[k] = S;
        }
    }
}

int lane_shift(int groups, int max_shift)
{
    int s = 0;
    while ((1 << s) < groups && s < max_shift) ++s;
    return s;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// part [slabs][B][C] and tot [B][C]: tot[b, c] = sum over v of a[b, v, c] (* m[b, v, c])
void colsum_run(hipStream_t sm, const float* a, const float* m, int B, int V, int C, double* part, double* tot)
{
    const int slabs = ceil_div(V, kSlab), nv = B * C;
    const bool vec = C % 4 == 0 && aligned16(a) && aligned16(m);
    // 8 lanes of 16 bytes (a 128-byte line) or 64 lanes of 4 per row of the workgroup
    const int groups = vec ? C / 4 : C, cshift = lane_shift(groups, vec ? 3 : 6);
    const dim3 grid((unsigned)slabs, (unsigned)B, (unsigned)ceil_div(groups, 1 << cshift));
    if (vec) {
        if (m) hipLaunchKernelGGL((colsum_kernel<4, true>), grid, dim3(256), 0, sm, a, m, V, C, cshift, part);
        else hipLaunchKernelGGL((colsum_kernel<4, false>), grid, dim3(256), 0, sm, a, m, V, C, cshift, part);
    } else {
        if (m) hipLaunchKernelGGL((colsum_kernel<1, true>), grid, dim3(256), 0, sm, a, m, V, C, cshift, part);
        else hipLaunchKernelGGL((colsum_kernel<1, false>), grid, dim3(256), 0, sm, a, m, V, C, cshift, part);
    }
    hipLaunchKernelGGL(reduce_partials_kernel<double>, dim3((unsigned)ceil_div(nv, 16)), dim3(256), 0, sm, part, slabs, nv, tot);
}

// ---- channel attention -------------------------------------------------------------------------------------------------------------------------

// One workgroup per sample; saliency.hip's ca_fold_kernel with the widths as arguments and the three vectors kept.
__global__ __launch_bounds__(256) void ca_dense_kernel(const double* __restrict__ tot, int V, int C, int Ch, const float* __restrict__ w1,
                                                       const float* __restrict__ b1, const float* __restrict__ w2, const float* __restrict__ b2,
                                                       float* __restrict__ mean_out, float* __restrict__ hidden_out, float* __restrict__ scale_out)
{
    __shared__ float mean[kMaxC], h[kMaxCh];
    const int t = threadIdx.x, b = blockIdx.x;
    for (int c = t; c < C; c += 256) {
        mean[c] = (float)(tot[(size_t)b * C + c] / V);
        mean_out[(size_t)b * C + c] = mean[c];
    }
    __syncthreads();
    for (int i = t; i < Ch; i += 256) {
        double acc = (double)b1[i];
        for (int c = 0; c < C; ++c) acc += (double)mean[c] * (double)w1[(size_t)c * Ch + i];
        h[i] = fmaxf((float)acc, 0.f);
        hidden_out[(size_t)b * Ch + i] = h[i];
    }
    __syncthreads();
    for (int c = t; c < C; c += 256) {
        double acc = (double)b2[c];
        for (int i = 0; i < Ch; ++i) acc += (double)h[i] * (double)w2[(size_t)i * C + c];
        scale_out[(size_t)b * C + c] = (float)(1.0 / (1.0 + exp(-acc)));
    }
}

// grid (ceil(V * C / VEC / 256), B): y = x * scale [+ add], scale and add per (sample, channel).  Every lane reads its own x before it
// writes y: y may be x.
template <int VEC, bool ADD>
__global__ __launch_bounds__(256) void ca_apply_kernel(const float* x, const float* __restrict__ scale, const float* __restrict__ add, int V, int C, float* y)
{
    const unsigned e = blockIdx.x * 256u + threadIdx.x, groups = (unsigned)C / VEC;
    if (e >= (unsigned)V * groups) return;
    const unsigned c = (e % groups) * VEC;
    const size_t i = (size_t)blockIdx.y * V * C + (size_t)e * VEC;
    const Vec<VEC> f = vload<VEC>(x + i), s = vload<VEC>(scale + (size_t)blockIdx.y * C + c);
    Vec<VEC> o;
    if (ADD) {
        const Vec<VEC> d = vload<VEC>(add + (size_t)blockIdx.y * C + c);
#pragma unroll
        for (int k = 0; k < VEC; ++k) o.v[k] = f.v[k] * s.v[k] + d.v[k];
    } else {
#pragma unroll
        for (int k = 0; k < VEC; ++k) o.v[k] = f.v[k] * s.v[k];
    }
    vstore<VEC>(y + i, o);
}

void ca_apply_run(hipStream_t sm, const float* x, const float* scale, const float* add, int B, int V, int C, float* y)
{
    const bool vec = C % 4 == 0 && aligned16(x) && aligned16(y) && aligned16(scale) && aligned16(add);
    const dim3 grid(blocks256((size_t)V * C / (vec ? 4 : 1)), (unsigned)B);
    if (vec) {
        if (add) hipLaunchKernelGGL((ca_apply_kernel<4, true>), grid, dim3(256), 0, sm, x, scale, add, V, C, y);
        else hipLaunchKernelGGL((ca_apply_kernel<4, false>), grid, dim3(256), 0, sm, x, scale, add, V, C, y);
    } else {
        if (add) hipLaunchKernelGGL((ca_apply_kernel<1, true>), grid, dim3(256), 0, sm, x, scale, add, V, C, y);
        else hipLaunchKernelGGL((ca_apply_kernel<1, false>), grid, dim3(256), 0, sm, x, scale, add, V, C, y);
    }
}

// The dense part of the backward, one workgroup: everything here is B * C * Ch products.  dz2 [B][C], dz1 [B][Ch] (float64) and
// dmv [B][C] = dmean / V (float32) live in scratch; a phase reads what the phase before it wrote, behind a barrier.
__global__ __launch_bounds__(256) void ca_bwd_dense_kernel(const double* __restrict__ ds, const float* __restrict__ mean, const float* __restrict__ hidden,
                                                           const float* __restrict__ scale, const float* __restrict__ w1, const float* __restrict__ w2,
                                                           int B, int V, int C, int Ch, double* dz2, double* dz1, float* dmv, float* __restrict__ dw1,
                                                           float* __restrict__ db1, float* __restrict__ dw2, float* __restrict__ db2)
{
    const int t = threadIdx.x;
    for (int e = t; e < B * C; e += 256) {
        const double s = (double)scale[e];
        dz2[e] = ds[e] * s * (1.0 - s);
    }
    __syncthreads();
    for (int e = t; e < B * Ch; e += 256) {
        const int b = e / Ch, i = e - b * Ch;
        double acc = 0.0;
        for (int c = 0; c < C; ++c) acc += (double)w2[(size_t)i * C + c] * dz2[(size_t)b * C + c];
        dz1[e] = hidden[e] > 0.f ? acc : 0.0;
    }
    __syncthreads();
    if (dw2)
        for (int e = t; e < Ch * C; e += 256) {
            const int i = e / C, c = e - i * C;
            double acc = 0.0;
            for (int b = 0; b < B; ++b) acc += (double)hidden[(size_t)b * Ch + i] * dz2[(size_t)b * C + c];
            dw2[e] = (float)acc;
        }
    if (db2)
        for (int c = t; c < C; c += 256) {
            double acc = 0.0;
            for (int b = 0; b < B; ++b) acc += dz2[(size_t)b * C + c];
            db2[c] = (float)acc;
        }
    if (dw1)
        for (int e = t; e < C * Ch; e += 256) {
            const int c = e / Ch, i = e - c * Ch;
            double acc = 0.0;
            for (int b = 0; b < B; ++b) acc += (double)mean[(size_t)b * C + c] * dz1[(size_t)b * Ch + i];
            dw1[e] = (float)acc;
        }
    if (db1)
        for (int i = t; i < Ch; i += 256) {
            double acc = 0.0;
            for (int b = 0; b < B; ++b) acc += dz1[(size_t)b * Ch + i];
            db1[i] = (float)acc;
        }
    if (dmv)
        for (int e = t; e < B * C; e += 256) {
            const int b = e / C, c = e - b * C;
            double acc = 0.0;
            for (int i = 0; i < Ch; ++i) acc += (double)w1[(size_t)c * Ch + i] * dz1[(size_t)b * Ch + i];
            dmv[e] = (float)(acc / V);
        }
}

// ---- spatial gate ------------------------------------------------------------------------------------------------------------------------------

// one lane per (row, VEC channels) of the B * V rows; as saliency.hip's sa_mul_kernel every lane of a row computes the row's sigmoid
template <int VEC>
__global__ __launch_bounds__(256) void gate_kernel(const float* __restrict__ a1, const float* __restrict__ a2, const float* __restrict__ a3, const float* f,
                                                   unsigned rows, int C, float* __restrict__ sa, float* y)
{
    const unsigned e = blockIdx.x * 256u + threadIdx.x, groups = (unsigned)C / VEC;
    const unsigned row = e / groups, cg = e - row * groups;
    if (row >= rows) return;
    const float z = (a1[row] + a2[row]) + a3[row];
    const float g = 1.f / (1.f + expf(-z));
    if (cg == 0) sa[row] = g;
    const size_t i = (size_t)row * C + (size_t)cg * VEC;
    const Vec<VEC> v = vload<VEC>(f + i);
    Vec<VEC> o;
#pragma unroll
    for (int k = 0; k < VEC; ++k) o.v[k] = v.v[k] * g;
    vstore<VEC>(y + i, o);
}

// A row is 1 << lshift lanes (a power of two up to 64, so a row never straddles a wave); lane l adds the channel groups l, l + lanes, ...
// in float64, the lanes meet in a butterfly: the order depends on C (and the alignment's VEC) alone.  df = dy * sa on the way.
template <int VEC>
__global__ __launch_bounds__(256) void gate_bwd_kernel(const float* dy, const float* __restrict__ f, const float* __restrict__ sa, unsigned rows, int C,
                                                       int lshift, float* df, float* __restrict__ da)
{
    const int lanes = 1 << lshift, lane = threadIdx.x & (lanes - 1), groups = C / VEC;
    const unsigned row = blockIdx.x * (256u >> lshift) + (threadIdx.x >> lshift);
    double acc = 0.0;
    float g = 0.f;
    if (row < rows) {
        g = sa[row];
        for (int cg = lane; cg < groups; cg += lanes) {
            const size_t i = (size_t)row * C + (size_t)cg * VEC;
            const Vec<VEC> d = vload<VEC>(dy + i), v = vload<VEC>(f + i);
#pragma unroll
            for (int k = 0; k < VEC; ++k) acc += (double)d.v[k] * (double)v.v[k];
            if (df) {
                Vec<VEC> o;
#pragma unroll
                for (int k = 0; k < VEC; ++k) o.v[k] = d.v[k] * g;
                vstore<VEC>(df + i, o);
            }
        }
    }
    if (da) {  // (uniform: every lane of the wave takes part in the exchange)
        for (int o = lanes >> 1; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
        if (lane == 0 && row < rows) da[row] = (float)((double)g * (1.0 - (double)g) * acc);
    }
}

// ---- softmax + weighted Dice -------------------------------------------------------------------------------------------------------------------

// How a voxel's C logits are moved.  MODE 2: C == 2, one 8-byte access; MODE 4: C % 4 == 0, 16-byte accesses; MODE 1: floats.
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

// saliency.hip's softmax_kernel on a row in registers
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

__device__ __forceinline__ double wave_sum(double a)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
    return a;
}

// grid (slabs, B): thread t adds the voxels v0 + t, v0 + t + 256, ... of its slab, the 64 lanes of a wave meet in a butterfly, the four
// waves are added ascending.  part [slab][B][C][3] = (S0, S1, S2).
template <int MODE>
__global__ __launch_bounds__(256) void dice_sums_kernel(const float* __restrict__ logits, const int* __restrict__ labels, const float* __restrict__ weight, int V,
                                                        int C, double* __restrict__ part)
{
    constexpr int NC = Row<MODE>::NC;
    __shared__ double red[4][3 * NC];
    const int t = threadIdx.x, b = blockIdx.y, v0 = blockIdx.x * kSlab, v1 = min(V, v0 + kSlab);
    double s0[NC], s1[NC], s2[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) s0[c] = s1[c] = s2[c] = 0.0;
    for (int v = v0 + t; v < v1; v += 256) {
        const size_t row = (size_t)b * V + v;
        Row<MODE> p;
        row_load<MODE>(logits + row * C, C, p);
        row_softmax<MODE>(C, p);
        const int g = labels[row];
        const double w = weight ? (double)weight[row] : 1.0;
#pragma unroll
        for (int c = 0; c < NC; ++c)
            if (c < C) {
                const double pc = (double)p.v[c];
                s1[c] += (w * pc) * pc;
                if (g == c) {
                    s0[c] += w * pc;
                    s2[c] += w;
                }
            }
    }
    const int wave = t >> 6;
#pragma unroll
    for (int c = 0; c < NC; ++c)
        if (c < C) {
            const double a0 = wave_sum(s0[c]), a1 = wave_sum(s1[c]), a2 = wave_sum(s2[c]);
            if ((t & 63) == 0) red[wave][c * 3] = a0, red[wave][c * 3 + 1] = a1, red[wave][c * 3 + 2] = a2;
        }
    __syncthreads();
    if (t < 3 * C) part[((size_t)blockIdx.x * gridDim.y + b) * 3 * C + t] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
}

// one thread: the loss from the sums, samples and classes ascending
__global__ void dice_finish_kernel(const double* __restrict__ sums, int B, int C, float* __restrict__ loss)
{
    if (blockIdx.x || threadIdx.x) return;
    double total = 0.0;
    for (int b = 0; b < B; ++b) {
        double score = 0.0;
        for (int c = 0; c < C; ++c) {
            const double* s = sums + ((size_t)b * C + c) * 3;
            score += 2.0 * s[0] / (s[1] + s[2] + 1e-5);
        }
        total += 1.0 - score / C;
    }
    *loss = (float)(total / B);
}

// grid (ceil(V / 256), B), a thread per voxel.  G_vc = w ([g = c] kA_c + kB_c p_vc) with kA_c = -k 2 / D_c, kB_c = k 2 num_c / D_c^2,
// k = dloss / (B C); past the softmax everything is float64, rounded once.  A thread reads its row before it writes it: dlogits may be logits.
template <int MODE>
__global__ __launch_bounds__(256) void dice_bwd_kernel(const float* logits, const int* __restrict__ labels, const float* __restrict__ weight,
                                                       const double* __restrict__ sums, const float* __restrict__ dloss, int B, int V, int C, float* dlogits)
{
    constexpr int NC = Row<MODE>::NC;
    __shared__ double kA[NC], kB[NC];
    const int t = threadIdx.x, b = blockIdx.y;
    if (t < C) {
        const double* s = sums + ((size_t)b * C + t) * 3;
        const double D = s[1] + s[2] + 1e-5, k = (dloss ? (double)*dloss : 1.0) / ((double)B * C);
        kA[t] = -k * 2.0 / D;
        kB[t] = k * 2.0 * (2.0 * s[0]) / (D * D);
    }
    __syncthreads();
    const int v = blockIdx.x * 256 + t;
    if (v >= V) return;
    const size_t row = (size_t)b * V + v;
    Row<MODE> p;
    row_load<MODE>(logits + row * C, C, p);
    row_softmax<MODE>(C, p);
    const int g = labels[row];
    const double w = weight ? (double)weight[row] : 1.0;
    double G[NC], dot = 0.0;
#pragma unroll
    for (int c = 0; c < NC; ++c)
        if (c < C) {
            const double pc = (double)p.v[c];
            G[c] = w * ((g == c ? kA[c] : 0.0) + kB[c] * pc);
            dot += pc * G[c];
        }
#pragma unroll
    for (int c = 0; c < NC; ++c)
        if (c < C) p.v[c] = (float)((double)p.v[c] * (G[c] - dot));
    row_store<MODE>(dlogits + row * C, C, p);
}

int dice_mode(int C, const void* a, const void* b)
{
    if (C == 2 && (reinterpret_cast<uintptr_t>(a) & 7) == 0 && (reinterpret_cast<uintptr_t>(b) & 7) == 0) return 2;
    if (C % 4 == 0 && aligned16(a) && aligned16(b)) return 4;
    return 1;
}

// ---- the argument checks -----------------------------------------------------------------------------------------------------------------------

int ca_shape_ok(const char* who, int64_t B, int64_t V, int64_t C, int64_t Ch)
{
    PS_CHECK(B >= 1 && B <= 65535, "%s: B = %lld, must be in [1, 65535]", who, (long long)B);
    PS_CHECK(C >= 1 && C <= kMaxC, "%s: C = %lld, must be in [1, %d]", who, (long long)C, kMaxC);
    PS_CHECK(Ch >= 1 && Ch <= kMaxCh, "%s: Ch = %lld, must be in [1, %d]", who, (long long)Ch, kMaxCh);
    PS_CHECK(V >= 1 && V < (1ll << 31) && V * C < (1ll << 31), "%s: V = %lld (V >= 1, V * C < 2^31)", who, (long long)V);
    return PS_OK;
}

int gate_shape_ok(const char* who, int64_t B, int64_t V, int64_t C)
{
    PS_CHECK(B >= 1 && B <= 65535, "%s: B = %lld, must be in [1, 65535]", who, (long long)B);
    PS_CHECK(C >= 1 && C <= kMaxC, "%s: C = %lld, must be in [1, %d]", who, (long long)C, kMaxC);
    PS_CHECK(V >= 1 && V < (1ll << 31) && B * V * C < (1ll << 31), "%s: V = %lld (V >= 1, B * V * C < 2^31)", who, (long long)V);
    return PS_OK;
}

int dice_shape_ok(const char* who, int64_t B, int64_t V, int64_t C)
{
    PS_CHECK(B >= 1 && B <= 65535, "%s: B = %lld, must be in [1, 65535]", who, (long long)B);
    PS_CHECK(C >= 2 && C <= kMaxClasses, "%s: C = %lld, must be in [2, %d]", who, (long long)C, kMaxClasses);
    PS_CHECK(V >= 1 && V < (1ll << 31), "%s: V = %lld, must be in [1, 2^31)", who, (long long)V);
    return PS_OK;
}

}  // namespace

}  // namespace ps

extern "C" int ps_channel_attention(ps_context* c, const void* x, int64_t B, int64_t V, int64_t C, int64_t Ch, const void* w1, const void* b1, const void* w2,
                                    const void* b2, void* mean, void* hidden, void* scale, void* y, void* scratch, int64_t* scratch_bytes)
{
    using namespace ps;
    static const char* who = "ps_channel_attention";
    PS_CHECK(scratch_bytes, "%s: NULL scratch_bytes", who);
    PS_TRY(ca_shape_ok(who, B, V, C, Ch));
    Carver cv{static_cast<char*>(scratch)};
    double* part = cv.take<double>((size_t)ceil_div(V, kSlab) * B * C);
    double* tot = cv.take<double>((size_t)B * C);
    if (!scratch) {
        *scratch_bytes = (int64_t)cv.off;
        return PS_OK;
    }
    PS_CHECK(x && w1 && b1 && w2 && b2, "%s: NULL x, w1, b1, w2 or b2 (they may be NULL only in the call that sizes the scratch)", who);
    PS_CHECK(mean && hidden && scale, "%s: NULL mean, hidden or scale (only y may be NULL)", who);
    PS_CHECK(c, "%s: NULL context", who);
    PS_TRY(check_scratch(who, scratch, scratch_bytes, cv.off));

    PS_HIP(hipSetDevice(c->device));
    hipStream_t sm = c->stream;
    Stage stg(c, "channel_attention", 4);
    const float* xf = static_cast<const float*>(x);
    colsum_run(sm, xf, nullptr, (int)B, (int)V, (int)C, part, tot);
    hipLaunchKernelGGL(ca_dense_kernel, dim3((unsigned)B), dim3(256), 0, sm, tot, (int)V, (int)C, (int)Ch, static_cast<const float*>(w1),
                       static_cast<const float*>(b1), static_cast<const float*>(w2), static_cast<const float*>(b2), static_cast<float*>(mean),
                       static_cast<float*>(hidden), static_cast<float*>(scale));
    if (y) ca_apply_run(sm, xf, static_cast<const float*>(scale), nullptr, (int)B, (int)V, (int)C, static_cast<float*>(y));
    PS_HIP(hipGetLastError());
    return PS_OK;
}

extern "C" int ps_channel_attention_bwd(ps_context* c, const void* x, const void* dy, const void* mean, const void* hidden, const void* scale, const void* w1,
                                        const void* w2, int64_t B, int64_t V, int64_t C, int64_t Ch, void* dx, void* dw1, void* db1, void* dw2, void* db2,
                                        void* scratch, int64_t* scratch_bytes)
{
    using namespace ps;
    static const char* who = "ps_channel_attention_bwd";
    PS_CHECK(scratch_bytes, "%s: NULL scratch_bytes", who);
    PS_TRY(ca_shape_ok(who, B, V, C, Ch));
    Carver cv{static_cast<char*>(scratch)};
    double* part = cv.take<double>((size_t)ceil_div(V, kSlab) * B * C);
    double* ds = cv.take<double>((size_t)B * C);
    double* dz2 = cv.take<double>((size_t)B * C);
    double* dz1 = cv.take<double>((size_t)B * Ch);
    float* dmv = cv.take<float>((size_t)B * C);
    if (!scratch) {
        *scratch_bytes = (int64_t)cv.off;
        return PS_OK;
    }
    PS_CHECK(x && dy && mean && hidden && scale && w1 && w2,
             "%s: NULL x, dy, mean, hidden, scale, w1 or w2 (they may be NULL only in the call that sizes the scratch)", who);
    PS_CHECK(dx || dw1 || db1 || dw2 || db2, "%s: every result is NULL", who);
    PS_CHECK(dx != x, "%s: dx must not overlap x (it may be dy)", who);
    PS_CHECK(c, "%s: NULL context", who);
    PS_TRY(check_scratch(who, scratch, scratch_bytes, cv.off));

    PS_HIP(hipSetDevice(c->device));
    hipStream_t sm = c->stream;
    Stage stg(c, "channel_attention_bwd", 4);
    const float *xf = static_cast<const float*>(x), *dyf = static_cast<const float*>(dy);
    colsum_run(sm, dyf, xf, (int)B, (int)V, (int)C, part, ds);
    hipLaunchKernelGGL(ca_bwd_dense_kernel, dim3(1), dim3(256), 0, sm, ds, static_cast<const float*>(mean), static_cast<const float*>(hidden),
                       static_cast<const float*>(scale), static_cast<const float*>(w1), static_cast<const float*>(w2), (int)B, (int)V, (int)C, (int)Ch, dz2,
                       dz1, dx ? dmv : nullptr, static_cast<float*>(dw1), static_cast<float*>(db1), static_cast<float*>(dw2), static_cast<float*>(db2));
    if (dx) ca_apply_run(sm, dyf, static_cast<const float*>(scale), dmv, (int)B, (int)V, (int)C, static_cast<float*>(dx));
    PS_HIP(hipGetLastError());
    return PS_OK;
}

extern "C" int ps_spatial_gate(ps_context* c, const void* a1, const void* a2, const void* a3, const void* f, int64_t B, int64_t V, int64_t C, void* sa, void* y)
{
    using namespace ps;
    static const char* who = "ps_spatial_gate";
    PS_TRY(gate_shape_ok(who, B, V, C));
    PS_CHECK(a1 && a2 && a3 && f && sa && y, "%s: NULL a1, a2, a3, f, sa or y", who);
    PS_CHECK(c, "%s: NULL context", who);

    PS_HIP(hipSetDevice(c->device));
    Stage stg(c, "spatial_gate", 1);
    const unsigned rows = (unsigned)(B * V);
    const bool vec = C % 4 == 0 && aligned16(f) && aligned16(y);
    const dim3 grid(blocks256((size_t)rows * C / (vec ? 4 : 1)));
    if (vec)
        hipLaunchKernelGGL(gate_kernel<4>, grid, dim3(256), 0, c->stream, static_cast<const float*>(a1), static_cast<const float*>(a2),
                           static_cast<const float*>(a3), static_cast<const float*>(f), rows, (int)C, static_cast<float*>(sa), static_cast<float*>(y));
    else
        hipLaunchKernelGGL(gate_kernel<1>, grid, dim3(256), 0, c->stream, static_cast<const float*>(a1), static_cast<const float*>(a2),
                           static_cast<const float*>(a3), static_cast<const float*>(f), rows, (int)C, static_cast<float*>(sa), static_cast<float*>(y));
    PS_HIP(hipGetLastError());
    return PS_OK;
}

extern "C" int ps_spatial_gate_bwd(ps_context* c, const void* dy, const void* f, const void* sa, int64_t B, int64_t V, int64_t C, void* df, void* da)
{
    using namespace ps;
    static const char* who = "ps_spatial_gate_bwd";
    PS_TRY(gate_shape_ok(who, B, V, C));
    PS_CHECK(dy && f && sa, "%s: NULL dy, f or sa", who);
    PS_CHECK(df || da, "%s: every result is NULL", who);
    PS_CHECK(df != f, "%s: df must not overlap f (it may be dy)", who);
    PS_CHECK(c, "%s: NULL context", who);

    PS_HIP(hipSetDevice(c->device));
    Stage stg(c, "spatial_gate_bwd", 1);
    const unsigned rows = (unsigned)(B * V);
    const bool vec = C % 4 == 0 && aligned16(dy) && aligned16(f) && aligned16(df);
    const int lshift = lane_shift((int)C / (vec ? 4 : 1), 6);
    const dim3 grid((unsigned)ceil_div(rows, 256 >> lshift));
    if (vec)
        hipLaunchKernelGGL(gate_bwd_kernel<4>, grid, dim3(256), 0, c->stream, static_cast<const float*>(dy), static_cast<const float*>(f),
                           static_cast<const float*>(sa), rows, (int)C, lshift, static_cast<float*>(df), static_cast<float*>(da));
    else
        hipLaunchKernelGGL(gate_bwd_kernel<1>, grid, dim3(256), 0, c->stream, static_cast<const float*>(dy), static_cast<const float*>(f),
                           static_cast<const float*>(sa), rows, (int)C, lshift, static_cast<float*>(df), static_cast<float*>(da));
    PS_HIP(hipGetLastError());
    return PS_OK;
}

extern "C" int ps_softmax_dice_loss(ps_context* c, const void* logits, const void* labels, const void* weight, int64_t B, int64_t V, int64_t C, void* loss,
                                    void* sums, void* scratch, int64_t* scratch_bytes)
{
    using namespace ps;
    static const char* who = "ps_softmax_dice_loss";
    PS_CHECK(scratch_bytes, "%s: NULL scratch_bytes", who);
    PS_TRY(dice_shape_ok(who, B, V, C));
    const int slabs = ceil_div(V, kSlab), nv = (int)(B * C * 3);
    Carver cv{static_cast<char*>(scratch)};
    double* part = cv.take<double>((size_t)slabs * nv);
    if (!scratch) {
        *scratch_bytes = (int64_t)cv.off;
        return PS_OK;
    }
    PS_CHECK(logits && labels, "%s: NULL logits or labels (they may be NULL only in the call that sizes the scratch; weight may be NULL)", who);
    PS_CHECK(loss && sums, "%s: NULL loss or sums", who);
    PS_CHECK(c, "%s: NULL context", who);
    PS_TRY(check_scratch(who, scratch, scratch_bytes, cv.off));

    PS_HIP(hipSetDevice(c->device));
    hipStream_t sm = c->stream;
    Stage stg(c, "softmax_dice_loss", 3);
    const float *lf = static_cast<const float*>(logits), *wf = static_cast<const float*>(weight);
    const int* gl = static_cast<const int*>(labels);
    const dim3 grid((unsigned)slabs, (unsigned)B);
    const int mode = dice_mode((int)C, logits, logits);
    if (mode == 2) hipLaunchKernelGGL(dice_sums_kernel<2>, grid, dim3(256), 0, sm, lf, gl, wf, (int)V, (int)C, part);
    else if (mode == 4) hipLaunchKernelGGL(dice_sums_kernel<4>, grid, dim3(256), 0, sm, lf, gl, wf, (int)V, (int)C, part);
    else hipLaunchKernelGGL(dice_sums_kernel<1>, grid, dim3(256), 0, sm, lf, gl, wf, (int)V, (int)C, part);
    hipLaunchKernelGGL(reduce_partials_kernel<double>, dim3((unsigned)ceil_div(nv, 16)), dim3(256), 0, sm, part, slabs, nv, static_cast<double*>(sums));
    hipLaunchKernelGGL(dice_finish_kernel, dim3(1), dim3(64), 0, sm, static_cast<const double*>(sums), (int)B, (int)C, static_cast<float*>(loss));
    PS_HIP(hipGetLastError());
    return PS_OK;
}

extern "C" int ps_softmax_dice_loss_bwd(ps_context* c, const void* logits, const void* labels, const void* weight, const void* sums, const void* dloss, int64_t B,
                                        int64_t V, int64_t C, void* dlogits)
{
    using namespace ps;
    static const char* who = "ps_softmax_dice_loss_bwd";
    PS_TRY(dice_shape_ok(who, B, V, C));
    PS_CHECK(logits && labels && sums, "%s: NULL logits, labels or sums (weight and dloss may be NULL)", who);
    PS_CHECK(dlogits, "%s: NULL dlogits", who);
    PS_CHECK(c, "%s: NULL context", who);

    PS_HIP(hipSetDevice(c->device));
    Stage stg(c, "softmax_dice_loss_bwd", 1);
    const float *lf = static_cast<const float*>(logits), *wf = static_cast<const float*>(weight), *dl = static_cast<const float*>(dloss);
    const int* gl = static_cast<const int*>(labels);
    const double* sd = static_cast<const double*>(sums);
    float* out = static_cast<float*>(dlogits);
    const dim3 grid((unsigned)ceil_div(V, 256), (unsigned)B);
    const int mode = dice_mode((int)C, logits, dlogits);
    if (mode == 2) hipLaunchKernelGGL(dice_bwd_kernel<2>, grid, dim3(256), 0, c->stream, lf, gl, wf, sd, dl, (int)B, (int)V, (int)C, out);
    else if (mode == 4) hipLaunchKernelGGL(dice_bwd_kernel<4>, grid, dim3(256), 0, c->stream, lf, gl, wf, sd, dl, (int)B, (int)V, (int)C, out);
    else hipLaunchKernelGGL(dice_bwd_kernel<1>, grid, dim3(256), 0, c->stream, lf, gl, wf, sd, dl, (int)B, (int)V, (int)C, out);
    PS_HIP(hipGetLastError());
    return PS_OK;
}
