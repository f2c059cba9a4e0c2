// dice_kit.h -- the two Dice kernels (the three per-class sums; the gradient from the sums), written once for the two losses that use them
// (DESIGN.md 4.21):
//
//   saliency network   softmax in front, a per-voxel weight map, hard or soft labels, [B] samples   saliency_train.hip
//   point network      the raw logits, validity of the label as the weight, u_c at the finish       point_loss.hip
//
// What differs is two compile-time policies.  ACT, the activation in front: forward(C, p) in place, backward(C, p, G, dot) turns
// G = dloss/dp into dloss/dlogit.  WT, where a row's weight comes from and what the finish makes of the sums: of(row, label, C);
// kValid: a weight of 0 drops the row before anything of it is read into a sum, and the rows that stay are counted (n_valid, n_correct:
// kExtra = 2 more sums behind the 3 C); WT::Finish, what the gradient pass makes of the sums: coef(...), a class's two gradient coefficients
// and its score from its three sums, and loss_of(...).
//
// The sums are float64: a partial per (slab of kSlab rows, sample, class), the threads of a slab added in a fixed order, the slabs by
// reduce_partials.h -- no float atomic, two runs give the same bytes.
#pragma once
#include "saliency_kit.h"

namespace ps {

__device__ __forceinline__ double wave_sum(double a)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
    return a;
}

// Where a voxel's label row g_vc comes from -- the one thing the hard-label and the soft-label (mixup, include/pointseg_saliency_mixup.h)
// forms of the two kernels below differ in.  at<MODE>(row, C) is voxel `row`; of it, has(c): g_vc can be non-zero, times(a, c) = a g_vc,
// asked once per class, ascending.  HardLabels: an integer g, g_vc = [g = c] -- a class that is not the voxel's adds nothing and a product
// by 1 is not made.  SoftLabels: C floats, moved like the logits (MODE 2: one 8-byte load; MODE 4: 16 bytes when the class enters a new
// four, so that only four are in registers beside the 16 logits; MODE 1: floats).  A product by exactly 0 or 1 and the addition of +0 to a
// float64 sum are exact, so one-hot soft rows give the bytes of the integer form.
struct HardLabels {
    const int* __restrict__ p;
    struct At {
        int g;
        __device__ __forceinline__ bool has(int c) const { return g == c; }
        __device__ __forceinline__ double times(double a, int) { return a; }
    };
    template <int MODE>
    __device__ __forceinline__ At at(size_t row, int) const
    {
        return At{p[row]};
    }
};

struct SoftLabels {
    const float* __restrict__ p;
    template <int MODE>
    struct At {
        const float* __restrict__ r;
        float q[MODE == 1 ? 1 : MODE];
        __device__ __forceinline__ bool has(int) const { return true; }
        __device__ __forceinline__ double times(double a, int c)
        {
            if (MODE == 1) return a * (double)r[c];
            if (MODE == 4 && (c & 3) == 0) {
                const float4 f = *reinterpret_cast<const float4*>(r + c);
                q[0] = f.x, q[1] = f.y, q[2] = f.z, q[3] = f.w;
            }
            return a * (double)q[c & (MODE - 1)];
        }
    };
    template <int MODE>
    __device__ __forceinline__ At<MODE> at(size_t row, int C) const
    {
        At<MODE> a;
        a.r = p + row * C;
        if (MODE == 2) {
            const float2 f = *reinterpret_cast<const float2*>(a.r);
            a.q[0] = f.x, a.q[1] = f.y;
        }
        return a;
    }
};

// ---- ACT: the activation in front of the Dice ------------------------------------------------------------------------------------------------

// p = softmax(logits); dlogit_c = p_c (G_c - sum_k p_k G_k), float64 past the softmax, rounded once
struct SoftmaxAct {
    template <int MODE>
    static __device__ __forceinline__ void forward(int C, Row<MODE>& p)
    {
        row_softmax<MODE>(C, p);
    }
    template <int MODE>
    static __device__ __forceinline__ void backward(int C, Row<MODE>& p, const double (&G)[Row<MODE>::NC], double dot)
    {
#pragma unroll
        for (int c = 0; c < Row<MODE>::NC; ++c)
            if (c < C) p.v[c] = (float)((double)p.v[c] * (G[c] - dot));
    }
};

// the Dice of the raw logits (PointSegment/RandLANet.py:276-312 has no softmax): dlogit_c = G_c, rounded once
struct NoAct {
    template <int MODE>
    static __device__ __forceinline__ void forward(int, Row<MODE>&)
    {
    }
    template <int MODE>
    static __device__ __forceinline__ void backward(int C, Row<MODE>& p, const double (&G)[Row<MODE>::NC], double)
    {
#pragma unroll
        for (int c = 0; c < Row<MODE>::NC; ++c)
            if (c < C) p.v[c] = (float)G[c];
    }
};

// tf.nn.in_top_k(row, g, 1) of row p whose target logit is zt: zt is finite and no class has a strictly larger logit (a tie is correct, a
// NaN elsewhere is not larger: fmaxf passes the other operand on).  The caller reads zt from memory -- picking it out of the registers
// costs a lane mask per class, and the sums kernel has no scalar registers to spare.
template <int MODE>
__device__ __forceinline__ bool row_top1(const Row<MODE>& p, float zt, int C)
{
    float m = zt;
#pragma unroll
    for (int c = 0; c < Row<MODE>::NC; ++c)
        if (c < C) m = fmaxf(m, p.v[c]);
    return fabsf(zt) < INFINITY && !(m > zt);  // (false for a NaN target too)
}

// ---- WT: a row's weight, and the finish -----------------------------------------------------------------------------------------------------

// a per-voxel map (NULL: ones) on both sides of the quotient; Finish: the loss is the mean over the B samples and the C classes, times *dloss
struct MapWeight {
    static constexpr int kExtra = 0;
    static constexpr bool kValid = false;
    const float* __restrict__ weight;
    template <class AT>
    __device__ __forceinline__ double of(size_t row, const AT&, int) const
    {
        return weight ? (double)weight[row] : 1.0;
    }
    template <int MODE, class AT>
    __device__ __forceinline__ bool correct(const Row<MODE>&, const float*, const AT&, int) const
    {
        return false;
    }
    struct Finish {
        const float* __restrict__ dloss;  // NULL: 1
        // G_vc = w (g_vc kA_c + kB_c p_vc) with kA_c = -k 2 / D_c, kB_c = k 2 num_c / D_c^2, k = dloss / (B C)
        __device__ __forceinline__ void coef(const double* __restrict__ s, int, int B, int C, double& kA, double& kB, double&) const
        {
            const double D = s[1] + s[2] + 1e-5, k = (dloss ? (double)*dloss : 1.0) / ((double)B * C);
            kA = -k * 2.0 / D;
            kB = k * 2.0 * (2.0 * s[0]) / (D * D);
        }
        __device__ __forceinline__ void loss_of(double, int) const {}
    };
};

// the point network's: a row counts iff its label is a class ([0, C); anything else is an ignored row, as for the cross-entropy).  Finish:
// the class weight u_c (NULL: ones) enters here: D_c = u_c S1_c + S2_c + 1e-5, s_c = 2 u_c S0_c / D_c, loss = 1 - mean_c s_c,
// dloss/dz_ic = g (b_c z_ic - a_c [y_i = c]) with a_c = 2 u_c / (C D_c), b_c = a_c s_c (include/pointseg_train_loss.h).
struct ValidWeight {
    static constexpr int kExtra = 2;
    static constexpr bool kValid = true;
    __device__ __forceinline__ double of(size_t, const HardLabels::At& y, int C) const { return (unsigned)y.g < (unsigned)C ? 1.0 : 0.0; }
    template <int MODE>
    __device__ __forceinline__ bool correct(const Row<MODE>& p, const float* z, const HardLabels::At& y, int C) const
    {
        return row_top1<MODE>(p, z[y.g], C);  // (z: the row in memory; y is a class here)
    }
    struct Finish {
        const float* __restrict__ u;
        double g;     // the grad scale
        float* loss;  // NULL: not wanted
        __device__ __forceinline__ void coef(const double* __restrict__ s, int c, int, int C, double& kA, double& kB, double& score) const
        {
            const double uc = u ? (double)u[c] : 1.0, D = uc * s[1] + s[2] + 1e-5, a = 2.0 * uc / ((double)C * D);
            score = 2.0 * uc * s[0] / D;
            kA = -g * a;
            kB = g * (a * score);
        }
        __device__ __forceinline__ void loss_of(double score_sum, int C) const
        {
            if (loss) *loss = (float)(1.0 - score_sum / (double)C);
        }
    };
};

// ---- the sums pass -----------------------------------------------------------------------------------------------------------------------------

// grid (slabs, B): thread t adds the voxels v0 + t, v0 + t + 256, ... of its slab, the 64 lanes of a wave meet in a butterfly, the four
// waves are added ascending.  part [slab][B][3 C + kExtra]: per class (S0, S1, S2), then (kValid) n_valid, n_correct -- exact integers.
template <int MODE, class LAB, class ACT, class WT>
__global__ __launch_bounds__(256) void dice_sums_kernel(const float* __restrict__ logits, LAB labels, WT wt, int V, int C, double* __restrict__ part)
{
    constexpr int NC = Row<MODE>::NC;
    __shared__ double red[4][3 * NC + WT::kExtra];
    const int t = threadIdx.x, b = blockIdx.y, v0 = blockIdx.x * kSlab, v1 = min(V, v0 + kSlab);
    double s0[NC], s1[NC], s2[NC], n0 = 0.0, n1 = 0.0;
#pragma unroll
    for (int c = 0; c < NC; ++c) s0[c] = s1[c] = s2[c] = 0.0;
    for (int v = v0 + t; v < v1; v += 256) {
        const size_t row = (size_t)b * V + v;
        Row<MODE> p;
        row_load<MODE>(logits + row * C, C, p);
        ACT::template forward<MODE>(C, p);
        auto g = labels.template at<MODE>(row, C);
        const double w = wt.of(row, g, C);
        if (WT::kValid) {
            if (w == 0.0) continue;
            n0 += 1.0;
            if (wt.template correct<MODE>(p, logits + row * C, g, C)) n1 += 1.0;
        }
#pragma unroll
        for (int c = 0; c < NC; ++c)
            if (c < C) {
                const double pc = (double)p.v[c];
                s1[c] += (w * pc) * pc;
                if (g.has(c)) {
                    const double wg = g.times(w, c);
                    s0[c] += wg * pc;
                    s2[c] += wg;
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
    if (WT::kValid) {
        const double a0 = wave_sum(n0), a1 = wave_sum(n1);
        if ((t & 63) == 0) red[wave][3 * C] = a0, red[wave][3 * C + 1] = a1;
    }
    __syncthreads();
    const int nv = 3 * C + WT::kExtra;
    if (t < nv) part[((size_t)blockIdx.x * gridDim.y + b) * nv + t] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
}

// ---- the from-sums pass ----------------------------------------------------------------------------------------------------------------------

// grid (ceil(V / 256), B), a thread per voxel.  G_vc = w (g_vc kA_c + kB_c p_vc), the coefficients in LDS from the sums (sample b's at
// sums + b 3 C); past the activation everything is float64, rounded once.  A thread reads its rows before it writes: dlogits may be
// logits.  kValid: thread 0 of the first workgroup hands the classes' scores to WT::Finish (the loss), a row of weight 0 gets zeros
// whatever its logits hold, and dlogits may be NULL (the loss alone, from one workgroup).
template <int MODE, class LAB, class ACT, class WT>
__global__ __launch_bounds__(256) void dice_bwd_kernel(const float* logits, LAB labels, WT wt, const double* __restrict__ sums,
                                                       typename WT::Finish fin, int B, int V, int C, float* dlogits)
{
    constexpr int NC = Row<MODE>::NC;
    __shared__ double kA[NC], kB[NC], sc[NC];
    const int t = threadIdx.x, b = blockIdx.y;
    if (t < C) {
        double score = 0.0;
        fin.coef(sums + ((size_t)b * C + t) * 3, t, B, C, kA[t], kB[t], score);
        if (WT::kValid) sc[t] = score;
    }
    __syncthreads();
    if (WT::kValid) {
        if (t == 0 && blockIdx.x == 0 && b == 0) {
            double total = 0.0;
            for (int c = 0; c < C; ++c) total += sc[c];
            fin.loss_of(total, C);
        }
        if (!dlogits) return;
    }
    const int v = blockIdx.x * 256 + t;
    if (v >= V) return;
    const size_t row = (size_t)b * V + v;
    Row<MODE> p;
    row_load<MODE>(logits + row * C, C, p);
    ACT::template forward<MODE>(C, p);
    auto g = labels.template at<MODE>(row, C);
    const double w = wt.of(row, g, C);
    double G[NC], dot = 0.0;
#pragma unroll
    for (int c = 0; c < NC; ++c)
        if (c < C) {
            const double pc = (double)p.v[c];
            G[c] = WT::kValid && w == 0.0 ? 0.0 : w * ((g.has(c) ? g.times(kA[c], c) : 0.0) + kB[c] * pc);
            dot += pc * G[c];
        }
    ACT::template backward<MODE>(C, p, G, dot);
    row_store<MODE>(dlogits + row * C, C, p);
}

}  // namespace ps
