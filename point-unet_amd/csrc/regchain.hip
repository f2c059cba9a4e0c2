// regchain.hip -- layer chains with the activations in REGISTERS between the layers (see rowgemm.h: rowchain).
//
// The chain is evaluated transposed: per 16-point tile a wave computes Y^T = W^T . X^T on v_mfma_f32_16x16x4_f32, A = a
// weight fragment, B = the activations.  In that orientation the accumulator layout of one layer IS the B-operand layout of the
// next: lane (point p = lane & 15, group g = lane >> 4) ends a layer holding output channels 16t + 4g + q (q = 0..3) of its
// point for every output tile t, and the k-step (t, q) of the next layer needs, from the same lane, exactly that value -- its
// four k-slots are then the channels {16t + q, 16t + 4 + q, 16t + 8 + q, 16t + 12 + q}, an order of the K axis like any other
// (the sum over k does not care; the weight fragments are laid out to match while they are staged into LDS).  So between two
// layers there is only bias + activation on the accumulator registers: no LDS round trip, no wave barrier, no re-layout.
// A lane's four channels of a tile are contiguous in memory, so inputs, appended sources and stored outputs are 16-byte
// accesses.  LDS holds the chain's weights (read once per workgroup, in k-step order: one conflict-free ds_read_b32 per MFMA).
// The tile counts of every layer are template parameters (the network uses seven chain shapes; any other chain takes the
// LDS-staged rowchain kernel), and the next tile's input rows are loaded before the current tile's MFMAs start.
//
// Reference formulation: helper_tf_util.conv2d / conv2d_transpose / tf.layers.dense on [B,N,1,C] tensors
// (PointSegment/helper_tf_util.py:115-250, RandLANet.py:113-151, 314-321), inference-mode BatchNorm folded on the host.
// Bound: HBM (only the chain's input rows and the rows somebody else reads cross it); fp32 MFMA for the widest chains.
//
// The frame (row loads, tile loop, bias + activation, stores) is written once; an OPERAND POLICY says how a layer's weights lie in LDS
// and how its products are issued.  RcF32 is the form above.  RcB3 runs the same products on v_mfma_f32_16x16x32_bf16 over exact
// three-way bfloat16 splits of both operands (b3_ops.h: six piece products per K = 32 step, fp32 accumulate, fp32-level error): the C
// layout of that instruction is the fp32 form's, and its B operand wants eight K values per lane -- the accumulators a lane holds of two
// adjacent 16-channel tiles -- so a k-step is a PAIR of input tiles (t, t + 1), its k-slot (g, j) the channel 16 (t + (j >> 2)) + 4 g +
// (j & 3), and a split in registers is all that stands between two layers.  The weights lie in LDS as three bfloat16 planes per
// (output tile, k-step): one conflict-free ds_read_b128 per plane and lane.  A chain with an odd input tile count stays on RcF32.
#include <algorithm>
#include <type_traits>

#include "b3_ops.h"
#include "mfma_tile.h"
#include "rowgemm.h"

namespace ps {

struct RcLayer {
    const float* wp;    // the layer's standard packed image (PackedLinear::wp, rowgemm.h); re-ordered while staged into LDS
    const float* bias;  // [>= ot*16]
    float* y;           // optional store of this layer's output rows
    const float* ex;    // optional plain-row source appended to the K axis (layer > 0)
    int ca, cb;         // channels of the two K segments: layer 0: s1 | s2; later: previous activations | ex
    int ta, tb;         // their tile counts
    int cout, ot;
    int ks, ntb;        // geometry of wp
    int ldy, ldex, leaky;
    int w_off, b_off;   // float offsets inside the workgroup's LDS image
};
struct RcArgs {
    const float* x1; const int32_t* g1; int ld1, g1m, g1n;
    const float* x2; const int32_t* g2; int ld2, g2m, g2n;
    int n, R;
    RcLayer l[kChainMaxSteps];
    const float* image;  // the chain's finished LDS image (weights in k-step order + biases), or nullptr: re-order while staging
    int image_floats;
};

// Chain shape: N layers; layer l reads IN(l) = (l == 0 ? A0 : O(l-1)) + B(l) sixteen-channel tiles and writes O(l).
template <int N_, int A0_, int B0_, int O0_, int B1_ = 0, int O1_ = 0, int B2_ = 0, int O2_ = 0, int B3_ = 0, int O3_ = 0>
struct RcShape {
    static constexpr int N = N_, A0 = A0_;
    static constexpr int B[4] = {B0_, B1_, B2_, B3_};
    static constexpr int O[4] = {O0_, O1_, O2_, O3_};
    static constexpr int A(int l) { return l == 0 ? A0_ : O[l - 1]; }
    static constexpr int IN(int l) { return A(l) + B[l]; }
    static constexpr int maxt()
    {
        int m = 1;
        for (int l = 0; l < N_; ++l) {
            m = IN(l) > m ? IN(l) : m;
            m = O[l] > m ? O[l] : m;
        }
        return m;
    }
};

// dst[T0 .. T0+NT)[q] <- channels 16(t - T0) + 4g + q of the row at rowp (zero beyond c).  Only the last tile can be partial.
template <int T0, int NT, int MT>
__device__ __forceinline__ void rc_load(float (&dst)[MT][4], const float* __restrict__ rowp, int c, bool vec, int g)
{
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int ch = t * 16 + 4 * g;
        if (vec) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (t + 1 < NT || ch < c) v = *reinterpret_cast<const float4*>(rowp + ch);
            dst[T0 + t][0] = v.x; dst[T0 + t][1] = v.y; dst[T0 + t][2] = v.z; dst[T0 + t][3] = v.w;
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) dst[T0 + t][q] = (t + 1 < NT || ch + q < c) ? rowp[ch + q] : 0.f;
        }
    }
}

// ---- operand policies: kThreads per workgroup, kPairFloats of LDS per (input tile, output tile) pair, mma = the products of one layer
// on the weights at wl, stage = one layer's weights from its standard packed image into the LDS image at dst (zero outside the layer) ----
struct RcF32 {
    static constexpr int kThreads = 256;
    static constexpr int kPairFloats = 256;
    template <int IT, int OT, int MT>
    static __device__ __forceinline__ void mma(f32x4 (&acc)[OT], const float (&act)[MT][4], const float* wl, int lane)
    {
        const float* w = wl + lane;
        // k-steps outermost: consecutive MFMAs go to different accumulators.  Wide layers go four output tiles at a time with a
        // scheduling fence between the groups: the compiler otherwise hoists every weight read of the layer in front of the first
        // MFMA (394 VGPRs, one wave per SIMD, for the 128-channel layer)
#pragma unroll
        for (int t0 = 0; t0 < OT; t0 += 4) {
#pragma unroll
            for (int ti = 0; ti < IT; ++ti)
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                    for (int to = t0; to < (t0 + 4 < OT ? t0 + 4 : OT); ++to)
                        acc[to] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[((to * IT + ti) * 4 + q) * 64], act[ti][q], acc[to], 0, 0, 0);
            if (t0 + 4 < OT) __builtin_amdgcn_sched_barrier(0);
        }
    }
    // dst[w_off + ((t_out * IT + t_in) * 4 + q) * 64 + lane] = W[k(t_in, lane >> 4, q)][16 t_out + (lane & 15)]
    static __device__ __forceinline__ void stage(const RcLayer& y, float* dst)
    {
        const int it_n = y.ta + y.tb;
        const int ln = threadIdx.x & 63, q = threadIdx.x >> 6;  // one (k-step, lane) slot per thread and (t_in, t_out) pair
        const int i = ln & 15, gg = ln >> 4;
        // eight pairs per round: the eight loads are issued before the first LDS store
        const int npairs = it_n * y.ot;
        for (int base = 0; base < npairs; base += 8) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int pr = base + u;
                v[u] = 0.f;
                if (pr < npairs) {
                    const int ti = pr / y.ot, to = pr - ti * y.ot;
                    int k;
                    bool kok;
                    if (ti < y.ta) { k = ti * 16 + 4 * gg + q; kok = k < y.ca; }
                    else { k = (ti - y.ta) * 16 + 4 * gg + q; kok = k < y.cb; k += y.ca; }
                    // wp[((cblk*KS + s)*64 + lane')*NTB + j] = W[s*4 + (lane' >> 4)][(cblk*NTB + j)*16 + (lane' & 15)]
                    const int cblk = to / y.ntb, j = to - cblk * y.ntb;
                    if (kok && to * 16 + i < y.cout) v[u] = y.wp[(((size_t)cblk * y.ks + (k >> 2)) * 64 + ((k & 3) * 16 + i)) * y.ntb + j];
                }
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int pr = base + u;
                if (pr < npairs) {
                    const int ti = pr / y.ot, to = pr - ti * y.ot;
                    dst[y.w_off + ((to * it_n + ti) * 4 + q) * 64 + ln] = v[u];
                }
            }
        }
    }
};

// RcPlanes<3> = RcB3 (above).  RcPlanes<1> = RcB1: ONE plane of operands rounded once to bfloat16 (round to nearest even), the policy of the
// chains whose layers all carry PackedLinear::round (PS_PREC_BF16) -- the same k-steps and layouts with one MFMA where RcB3 has six, and an
// image of 2 bytes per weight (the widest chain, RcPair2: 32 KB where the fp32 image has 64 KB).
template <int P>
struct RcPlanes {
    // (P = 3: eight waves share one image: it is 1.5x the fp32 one, and the widest chain's 97 KB leave room for one workgroup per CU.
    //  P = 1: the image is a third of that and two workgroups of eight waves would fit the LDS, but rc_blocks caps a CU at 16 waves, which
    //  the chains' register counts (above 64) already make two waves per SIMD: eight waves per workgroup, two workgroups per CU)
    static constexpr int kThreads = 512;
    static constexpr int kPairFloats = 128 * P;  // 16 x 16 weights of 2 P bytes
    template <int IT, int OT, int MT>
    static __device__ __forceinline__ void mma(f32x4 (&acc)[OT], const float (&act)[MT][4], const float* wl, int lane)
    {
        static_assert(IT % 2 == 0, "a k-step of the split-bf16 policy is a pair of 16-channel tiles");
        constexpr int KP = IT / 2;
        const uint4* w = reinterpret_cast<const uint4*>(wl) + lane;
        BPlanes<P> b[KP];
#pragma unroll
        for (int kp = 0; kp < KP; ++kp)
            b[kp] = b3_split8<P>(make_float4(act[2 * kp][0], act[2 * kp][1], act[2 * kp][2], act[2 * kp][3]),
                                 make_float4(act[2 * kp + 1][0], act[2 * kp + 1][1], act[2 * kp + 1][2], act[2 * kp + 1][3]));
        // (four output tiles at a time with a scheduling fence between the groups, as in RcF32)
#pragma unroll
        for (int t0 = 0; t0 < OT; t0 += 4) {
#pragma unroll
            for (int kp = 0; kp < KP; ++kp)
#pragma unroll
                for (int to = t0; to < (t0 + 4 < OT ? t0 + 4 : OT); ++to) {
                    BPlanes<P> a;
#pragma unroll
                    for (int pl = 0; pl < P; ++pl) a.p[pl] = w[((to * KP + kp) * P + pl) * 64];
                    acc[to] = b3_mfma16_6(a, b[kp], acc[to]);
                }
            if (t0 + 4 < OT) __builtin_amdgcn_sched_barrier(0);
        }
    }
    // 16-byte words: dst[w_off / 4 + ((t_out * KP + kp) * P + plane) * 64 + lane] = plane of the eight weights
    // W[k(2 kp + (e >> 2), lane >> 4, e & 3)][16 t_out + (lane & 15)], e = 0..7
    static __device__ __forceinline__ void stage(const RcLayer& y, float* dst)
    {
        const int kp_n = (y.ta + y.tb) / 2;
        uint4* out = reinterpret_cast<uint4*>(dst + y.w_off);
        for (int s = threadIdx.x; s < y.ot * kp_n * 64; s += kThreads) {
            const int ln = s & 63, slot = s >> 6;
            const int to = slot / kp_n, kp = slot - to * kp_n;
            const int i = ln & 15, gg = ln >> 4;
            const int cblk = to / y.ntb, j = to - cblk * y.ntb;
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int ti = 2 * kp + (e >> 2), q = e & 3;
                int k;
                bool kok;
                if (ti < y.ta) { k = ti * 16 + 4 * gg + q; kok = k < y.ca; }
                else { k = (ti - y.ta) * 16 + 4 * gg + q; kok = k < y.cb; k += y.ca; }
                v[e] = 0.f;
                if (kok && to * 16 + i < y.cout) v[e] = y.wp[(((size_t)cblk * y.ks + (k >> 2)) * 64 + ((k & 3) * 16 + i)) * y.ntb + j];
            }
            const BPlanes<P> p = b3_split8<P>(v);
#pragma unroll
            for (int pl = 0; pl < P; ++pl) out[(slot * P + pl) * 64 + ln] = p.p[pl];
        }
    }
};
using RcB3 = RcPlanes<3>;
using RcB1 = RcPlanes<1>;

template <class S, class P, int L>
__device__ __forceinline__ void rc_layer(const RcArgs& a, float (&act)[S::maxt()][4], const float* lds, int lane, int g, int row, int rr, bool ok)
{
    if constexpr (L < S::N) {
        constexpr int IT = S::IN(L), OT = S::O[L], TA = S::A(L), TB = S::B[L];
        const RcLayer& y = a.l[L];
        if constexpr (L > 0 && TB > 0) {
            const bool ve = (y.cb & 3) == 0 && (y.ldex & 3) == 0 && (reinterpret_cast<uintptr_t>(y.ex) & 15) == 0;
            rc_load<TA, TB>(act, y.ex + (size_t)rr * y.ldex, y.cb, ve, g);
        }
        f32x4 acc[OT];
#pragma unroll
        for (int to = 0; to < OT; ++to) acc[to] = f32x4{0.f, 0.f, 0.f, 0.f};
        if constexpr (L > 0) __builtin_amdgcn_sched_barrier(0);  // keep this layer's weight reads behind the previous layer's MFMAs
        P::template mma<IT, OT>(acc, act, lds + y.w_off, lane);
        const bool vy = y.y && (y.cout & 3) == 0 && (y.ldy & 3) == 0 && (reinterpret_cast<uintptr_t>(y.y) & 15) == 0;
#pragma unroll
        for (int to = 0; to < OT; ++to) {
            const int ch = to * 16 + 4 * g;
            const float4 b = *reinterpret_cast<const float4*>(lds + y.b_off + ch);  // zero on padding channels, like the weights
            float v[4] = {acc[to][0] + b.x, acc[to][1] + b.y, acc[to][2] + b.z, acc[to][3] + b.w};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (y.leaky) v[q] = leaky02(v[q]);
                act[to][q] = v[q];
            }
            if (y.y && ok) {
                float* o = y.y + (size_t)row * y.ldy + ch;
                if (vy) {
                    if (to + 1 < OT || ch < y.cout) *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (to + 1 < OT || ch + q < y.cout) o[q] = v[q];
                }
            }
        }
        rc_layer<S, P, L + 1>(a, act, lds, lane, g, row, rr, ok);
    }
}

// The chain's LDS image: per layer the weights in the policy's k-step order (zero outside the layer), then the biases.  One workgroup of
// P::kThreads threads.
template <class P>
__device__ __forceinline__ void rc_stage(const RcArgs& a, float* dst)
{
    for (int l = 0; l < a.n; ++l) {
        const RcLayer& y = a.l[l];
        P::stage(y, dst);
        for (int e = threadIdx.x; e < y.ot * 16; e += P::kThreads) dst[y.b_off + e] = e < y.cout ? y.bias[e] : 0.f;
    }
}

template <class P>
__global__ __launch_bounds__(P::kThreads) void rc_pack_kernel(RcArgs a, float* out) { rc_stage<P>(a, out); }

template <class S, class P>
__global__ __launch_bounds__(P::kThreads) void regchain_kernel(RcArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float rc_lds[];
    constexpr int MT = S::maxt(), WAVES = P::kThreads / 64;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int p = lane & 15, g = lane >> 4;
    if (a.image) {  // built once per network by rc_pack_kernel: a plain 16-byte copy
        for (int i = threadIdx.x; i < a.image_floats / 4; i += P::kThreads) reinterpret_cast<float4*>(rc_lds)[i] = reinterpret_cast<const float4*>(a.image)[i];
    } else {
        rc_stage<P>(a, rc_lds);
    }
    __syncthreads();

    const bool v1 = (a.l[0].ca & 3) == 0 && (a.ld1 & 3) == 0 && (reinterpret_cast<uintptr_t>(a.x1) & 15) == 0;
    const bool v2 = (a.l[0].cb & 3) == 0 && (a.ld2 & 3) == 0 && (reinterpret_cast<uintptr_t>(a.x2) & 15) == 0;
    const int stride = gridDim.x * WAVES;
    // rows past the end are computed on a copy of the last row (loads never leave the buffers) and not stored
    auto load_inputs = [&](int tile, float (&dst)[MT][4]) {
        const int rr = min(tile * 16 + p, a.R - 1);
        const int s1 = a.g1 ? (a.g1m ? (rr / a.g1m) * a.g1n : 0) + a.g1[rr] : rr;
        rc_load<0, S::A0>(dst, a.x1 + (size_t)s1 * a.ld1, a.l[0].ca, v1, g);
        if constexpr (S::B[0] > 0) {
            const int s2 = a.g2 ? (a.g2m ? (rr / a.g2m) * a.g2n : 0) + a.g2[rr] : rr;
            rc_load<S::A0, S::B[0]>(dst, a.x2 + (size_t)s2 * a.ld2, a.l[0].cb, v2, g);
        }
    };
    int tile = blockIdx.x * WAVES + wave;
    float act[MT][4], nxt[MT][4];
    if (tile * 16 < a.R) load_inputs(tile, nxt);
    for (; tile * 16 < a.R; tile += stride) {
#pragma unroll
        for (int t = 0; t < S::IN(0); ++t)
#pragma unroll
            for (int q = 0; q < 4; ++q) act[t][q] = nxt[t][q];
        if ((tile + stride) * 16 < a.R) load_inputs(tile + stride, nxt);  // in flight under this tile's MFMAs
        const int row = tile * 16 + p;
        rc_layer<S, P, 0>(a, act, rc_lds, lane, g, row, min(row, a.R - 1), row < a.R);
    }
}

static inline int rc_tiles(int c) { return (c + 15) / 16; }

// the chain shapes of the network (BraTS and Pancreas configurations): see the launch plan in randla.hip
using RcFc0 = RcShape<2, 1, 0, 1, 0, 1>;              // fc0 -> mlp1 (level 0): <=16 -> 8 -> 8
using RcEnc0 = RcShape<2, 1, 0, 1, 1, 2>;             // level 0: att2-mlp 16 -> 16, then [16 | shortcut 8] -> 32
using RcOne0 = RcShape<1, 1, 0, 1>;                   // level 0: att1-mlp 16 -> 8 (a single layer: no pre-product at d = 16)
using RcPair1 = RcShape<2, 2, 0, 2, 0, 4>;            // level 1: mlp1 32 -> 32, G = f . Wfc[:32] 32 -> 64
using RcPair1b = RcShape<2, 4, 0, 2, 0, 4>;           // level 1: att1-mlp 64 -> 32, G 32 -> 64
using RcEnc1 = RcShape<2, 4, 0, 4, 2, 8>;             // level 1: att2-mlp 64 -> 64, then [64 | shortcut 32] -> 128
using RcPair2 = RcShape<2, 8, 0, 4, 0, 8>;            // level 2: mlp1 / att1-mlp 128 -> 64, G = f . Wfc[:64] 64 -> 128 (64 KB of weights)
using RcHead = RcShape<4, 2, 2, 2, 0, 4, 0, 2, 0, 1>;  // [skip 32 | up 32] -> 32 -> 64 -> 32 -> classes

template <class S>
static bool rc_matches(const RcArgs& a)
{
    if (a.n != S::N) return false;
    for (int l = 0; l < S::N; ++l)
        if (a.l[l].ta != S::A(l) || a.l[l].tb != S::B[l] || a.l[l].ot != S::O[l]) return false;
    return true;
}

// The chains that take the split-bf16 policy when the context's regchain_b3 is on: those whose own kernel measured faster than the fp32 one by
// more than its run-to-run spread: the head, level 1's three chains.  RcPair2 (level 2: 704 tiles, 88 workgroups of eight
// waves) measured inside the spread and stays on fp32, as do the HBM-bound level-0 shapes and every shape with an odd input tile count.
template <class S>
constexpr bool rc_even_inputs()
{
    for (int l = 0; l < S::N; ++l)
        if (S::IN(l) & 1) return false;
    return true;
}
template <class S>
constexpr bool kRcSplit = std::is_same<S, RcHead>::value || std::is_same<S, RcEnc1>::value || std::is_same<S, RcPair1>::value ||
                          std::is_same<S, RcPair1b>::value;

// The chains that take the one-plane policy when every layer's operands are rounded (PackedLinear::round): every compiled shape whose K axes
// come in pairs of 16-channel tiles -- the four above and level 2's RcPair2.  The rule is per layer and the policy per chain: a chain that mixes
// rounded and unrounded layers, or a rounded one of another shape, is none of regchain's (rc_build) and runs on rowchain_kernel or layer by layer,
// which round per layer.
template <class S>
constexpr bool kRcOnePlane = kRcSplit<S> || std::is_same<S, RcPair2>::value;

// the float offsets of every layer inside the LDS image of a policy; returns the image's bytes
static size_t rc_layout(RcArgs& a, int pair_floats)
{
    int off = 0;
    for (int i = 0; i < a.n; ++i) {
        RcLayer& y = a.l[i];
        y.w_off = off; off += y.ot * (y.ta + y.tb) * pair_floats;
        y.b_off = off; off += y.ot * 16;
    }
    return (size_t)off * sizeof(float);
}

// (the offsets and lds_bytes are those of the fp32 policy, or of the one-plane policy when `rounded` comes back set: what the context-free plan reports)
static bool rc_build(const ChainStep* steps, int n_steps, const RowSrc& s1, const RowSrc& s2, RcArgs& a, size_t& lds_bytes, bool& rounded)
{
    rounded = false;
    if (n_steps < 1 || n_steps > kChainMaxSteps) return false;
    a = RcArgs{};
    a.x1 = s1.x; a.g1 = s1.gather; a.ld1 = s1.ld; a.g1m = s1.gm; a.g1n = s1.gn;
    a.x2 = s2.x; a.g2 = s2.gather; a.ld2 = s2.ld; a.g2m = s2.gm; a.g2n = s2.gn;
    a.n = n_steps;
    int prev = 0;
    for (int i = 0; i < n_steps; ++i) {
        const PackedLinear* L = steps[i].L;
        if (!L || !L->wp || !L->bias) return false;
        if (steps[i].extra.x && (i == 0 || steps[i].extra.gather)) return false;
        RcLayer& y = a.l[i];
        y.wp = L->wp; y.bias = L->bias; y.y = steps[i].y; y.ldy = steps[i].ldy;
        y.ex = i > 0 ? steps[i].extra.x : nullptr; y.ldex = steps[i].extra.ld;
        y.ca = i == 0 ? s1.c : prev;
        y.cb = i == 0 ? s2.c : (steps[i].extra.x ? steps[i].extra.c : 0);
        if (y.ca + y.cb != L->cin) return false;
        y.ta = rc_tiles(y.ca); y.tb = rc_tiles(y.cb);
        y.cout = L->cout; y.ot = rc_tiles(L->cout);
        y.ks = L->ks; y.ntb = L->ntb; y.leaky = L->leaky;
        prev = L->cout;
    }
    int n_round = 0;
    for (int i = 0; i < n_steps; ++i) n_round += steps[i].L->round != 0;
    if (n_round) {  // rounded operands: all layers or none, and only the shapes of the one-plane policy
        if (n_round != n_steps) return false;
        rounded = true;
        lds_bytes = rc_layout(a, RcB1::kPairFloats);
        return rc_matches<RcPair1>(a) || rc_matches<RcPair1b>(a) || rc_matches<RcEnc1>(a) || rc_matches<RcPair2>(a) || rc_matches<RcHead>(a);
    }
    lds_bytes = rc_layout(a, RcF32::kPairFloats);
    return rc_matches<RcFc0>(a) || rc_matches<RcEnc0>(a) || rc_matches<RcOne0>(a) || rc_matches<RcPair1>(a) || rc_matches<RcPair1b>(a) ||
           rc_matches<RcEnc1>(a) || rc_matches<RcPair2>(a) || rc_matches<RcHead>(a);
}

bool regchain_fits(const ChainStep* steps, int n_steps, const RowSrc& s1, const RowSrc& s2)
{
    RcArgs a;
    size_t lds = 0;
    bool rounded = false;
    return rc_build(steps, n_steps, s1, s2, a, lds, rounded);
}

static int rc_blocks(int64_t R, size_t lds_bytes, int waves)
{
    const int64_t tiles = (R + 15) / 16;
    // weights staged once per workgroup; at most 16 waves per CU (every chain kernel needs more than 64 VGPRs at its widest)
    const int per_cu = std::max(1, std::min(16 / waves, (int)(160 * 1024 / std::max<size_t>(lds_bytes, 1))));
    return (int)std::max<int64_t>(1, std::min<int64_t>((tiles + waves - 1) / waves, 256 * per_cu));
}

ChainPlan regchain_plan(const ChainStep* steps, int n_steps, const RowSrc& s1, const RowSrc& s2, int64_t R)
{
    ChainPlan p;
    RcArgs a;
    bool rounded = false;
    if (!rc_build(steps, n_steps, s1, s2, a, p.lds_bytes, rounded)) return ChainPlan();
    p.form = rounded ? 3 : 1;
    p.blocks = rc_blocks(R, p.lds_bytes, (rounded ? RcB1::kThreads : RcF32::kThreads) / 64);
    return p;
}

// one chain on one policy: the policy's image layout, the cached (or in-kernel) image, the launch
template <class S, class P>
static int rc_run(ps_context* c, RcArgs& a, ChainCache* cache)
{
    constexpr int policy = std::is_same<P, RcB3>::value ? 1 : (std::is_same<P, RcB1>::value ? 2 : 0);
    const size_t lds_bytes = rc_layout(a, P::kPairFloats);
    if (cache) {
        // the re-ordered weight image depends only on the layers, the split of the first K axis and the policy: build it once per network
        ChainCache::Entry* hit = nullptr;
        for (auto& e : cache->entries)
            if (e.wp0 == a.l[0].wp && e.wp_last == a.l[a.n - 1].wp && e.n == a.n && e.ca == a.l[0].ca && e.cb == a.l[0].cb && e.policy == policy) hit = &e;
        if (!hit) {
            cache->entries.emplace_back();
            hit = &cache->entries.back();
            hit->wp0 = a.l[0].wp; hit->wp_last = a.l[a.n - 1].wp; hit->n = a.n; hit->ca = a.l[0].ca; hit->cb = a.l[0].cb; hit->policy = policy;
            PS_TRY(hit->img.reserve(lds_bytes));
            hipLaunchKernelGGL(rc_pack_kernel<P>, dim3(1), dim3(P::kThreads), 0, c->stream, a, hit->img.as<float>());
            PS_HIP(hipGetLastError());
        }
        a.image = hit->img.as<float>();
        a.image_floats = (int)(lds_bytes / sizeof(float));
    }
    // dynamic LDS above the default limit: raised once per kernel and device (a context is bound to one device)
    size_t& have = c->regchain_lds_attr[reinterpret_cast<const void*>(regchain_kernel<S, P>)];
    if (lds_bytes > 48 * 1024 && lds_bytes > have) {
        PS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(regchain_kernel<S, P>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
        have = lds_bytes;
    }
    hipLaunchKernelGGL((regchain_kernel<S, P>), dim3(rc_blocks(a.R, lds_bytes, P::kThreads / 64)), dim3(P::kThreads), lds_bytes, c->stream, a);
    PS_HIP(hipGetLastError());
    return PS_OK;
}

template <class S>
static int rc_route(ps_context* c, RcArgs& a, ChainCache* cache, bool rounded)
{
    if constexpr (kRcOnePlane<S>) {
        static_assert(rc_even_inputs<S>(), "the one-plane policy takes its K axis in pairs of 16-channel tiles");
        if (rounded) return rc_run<S, RcB1>(c, a, cache);  // (whatever the context's regchain_b3 says: that switch is the default precision's)
    }
    if constexpr (kRcSplit<S>) {
        static_assert(rc_even_inputs<S>(), "the split-bf16 policy takes its K axis in pairs of 16-channel tiles");
        if (c->regchain_b3) return rc_run<S, RcB3>(c, a, cache);
    }
    return rc_run<S, RcF32>(c, a, cache);
}

int regchain(ps_context* c, const ChainStep* steps, int n_steps, const RowSrc& s1, const RowSrc& s2, int64_t R, ChainCache* cache)
{
    if (R <= 0) return PS_OK;
    RcArgs a;
    size_t lds_bytes = 0;
    bool rounded = false;
    PS_CHECK(rc_build(steps, n_steps, s1, s2, a, lds_bytes, rounded), "regchain: not one of the compiled chain shapes");
    PS_CHECK(R < (int64_t)1 << 31, "regchain: too many rows");
    a.R = (int)R;
    if (rc_matches<RcFc0>(a)) return rc_route<RcFc0>(c, a, cache, rounded);
    if (rc_matches<RcEnc0>(a)) return rc_route<RcEnc0>(c, a, cache, rounded);
    if (rc_matches<RcOne0>(a)) return rc_route<RcOne0>(c, a, cache, rounded);
    if (rc_matches<RcPair1>(a)) return rc_route<RcPair1>(c, a, cache, rounded);
    if (rc_matches<RcPair1b>(a)) return rc_route<RcPair1b>(c, a, cache, rounded);
    if (rc_matches<RcEnc1>(a)) return rc_route<RcEnc1>(c, a, cache, rounded);
    if (rc_matches<RcPair2>(a)) return rc_route<RcPair2>(c, a, cache, rounded);
    return rc_route<RcHead>(c, a, cache, rounded);
}

}  // namespace ps
