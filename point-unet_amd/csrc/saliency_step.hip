// saliency_step.hip -- the training step of the saliency attention network behind one call (include/pointseg_saliency_step.h, DESIGN.md
// 4.13): a graph walker over the ops of saliency.hip, conv3d.hip, conv3d_train.hip and saliency_train.hip, reached through their C entry
// points -- each checks its own limits and carves its own scratch, so the walker adds no second form of any of them and their code
// objects stay what they are -- and the two kernels torch stood in for: the strided copy / add and the momentum update.
//
// The walker runs twice over the same code: once with `run` off, where every op only reports its scratch (and refuses a shape it cannot
// take, before anything is enqueued), once enqueueing.  Where everything lies is saliency_step_plan.h's, a function of the shapes.
//
// The convolutions run at one precision per role -- forward, data gradient, weight gradient -- through the _prec entries of their ops
// (include/pointseg_saliency_step_precision.h); PS_PREC_FP32 three times is the step as it was, byte for byte.
#include <algorithm>

#include "../../include/pointseg_saliency_attention.h"
#include "../../include/pointseg_saliency_mixup.h"
#include "../../include/pointseg_saliency_step.h"
#include "../../include/pointseg_saliency_step_precision.h"
#include "../../include/pointseg_saliency_train.h"
#include "common.h"
#include "saliency.h"
#include "saliency_kit.h"
#include "saliency_step_plan.h"

namespace ps {

namespace {

// ---- the strided copy / add ------------------------------------------------------------------------------------------------------------------

// dst[r, 0:C] = a[r, 0:C] (+ b[r, 0:C]) over `rows` voxels, the three at channel pitches ldd, lda, ldb: a concat part into its concat,
// a concat's gradient out of it, the residual add, and the sum of two gradients.  One lane per (voxel, VEC channels); a lane reads its
// own elements before it writes them: dst may be a or b.
template <int VEC, bool ADD>
__global__ __launch_bounds__(256) void cols_kernel(const float* a, int lda, const float* b, int ldb, size_t rows, int C, float* dst, int ldd)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    const unsigned groups = (unsigned)C / VEC;
    const size_t r = e / groups;
    if (r >= rows) return;
    const unsigned c = (unsigned)(e - r * groups) * VEC;
    Vec<VEC> f = vload<VEC>(a + r * lda + c);
    if (ADD) {
        const Vec<VEC> g = vload<VEC>(b + r * ldb + c);
#pragma unroll
        for (int k = 0; k < VEC; ++k) f.v[k] = f.v[k] + g.v[k];
    }
    vstore<VEC>(dst + r * ldd + c, f);
}

void cols_run(hipStream_t sm, const float* a, int lda, const float* b, int ldb, size_t rows, int C, float* dst, int ldd)
{
    const bool vec = C % 4 == 0 && lda % 4 == 0 && ldd % 4 == 0 && (!b || ldb % 4 == 0) && aligned16(a) && aligned16(b) && aligned16(dst);
    const dim3 grid(blocks256(rows * (size_t)(C / (vec ? 4 : 1))));
    if (vec) {
        if (b) hipLaunchKernelGGL((cols_kernel<4, true>), grid, dim3(256), 0, sm, a, lda, b, ldb, rows, C, dst, ldd);
        else hipLaunchKernelGGL((cols_kernel<4, false>), grid, dim3(256), 0, sm, a, lda, b, ldb, rows, C, dst, ldd);
    } else {
        if (b) hipLaunchKernelGGL((cols_kernel<1, true>), grid, dim3(256), 0, sm, a, lda, b, ldb, rows, C, dst, ldd);
        else hipLaunchKernelGGL((cols_kernel<1, false>), grid, dim3(256), 0, sm, a, lda, b, ldb, rows, C, dst, ldd);
    }
}

// ---- the update --------------------------------------------------------------------------------------------------------------------------------

// how many of the table's bounds are <= e0 + k, for the VEC elements of a piece in one walk over the table: odd inside a kernel tensor.
// Every index is a constant: the table stays in kernel-argument memory.
template <int VEC>
__device__ __forceinline__ void bounds_below(const DecayTable& t, int e0, int (&n)[VEC])
{
#pragma unroll
    for (int k = 0; k < VEC; ++k) n[k] = 0;
#pragma unroll
    for (int j = 0; j < 96; ++j) {
        const int d = t.bound[j] - e0;  // (both below 2^31 and >= 0: no overflow)
#pragma unroll
        for (int k = 0; k < VEC; ++k) n[k] += d <= k ? 1 : 0;
    }
}

__device__ __forceinline__ void sgd_element(float& w, float g, float& acc, bool decay, float lr, float mom, float l2, float gs)
{
    g = __fmul_rn(g, gs);
    if (decay) g = __fadd_rn(g, __fmul_rn(l2, w));
    acc = __fadd_rn(__fmul_rn(mom, acc), g);
    w = __fsub_rn(w, __fmul_rn(lr, acc));
}

// One lane per piece of VEC elements; the last piece of a buffer whose length is no multiple of VEC goes a float at a time.
template <int VEC>
__global__ __launch_bounds__(256) void sgd_update_kernel(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ acc, int n, DecayTable t,
                                                         float lr, float mom, float l2, float gs)
{
    const int64_t e64 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * VEC;
    if (e64 >= n) return;
    const int e0 = (int)e64;
    int nb[VEC];
    bounds_below<VEC>(t, e0, nb);
    if (VEC == 4 && e0 + 4 <= n) {
        Vec<VEC> wv = vload<VEC>(w + e0), av = vload<VEC>(acc + e0);
        const Vec<VEC> gv = vload<VEC>(g + e0);
#pragma unroll
        for (int k = 0; k < VEC; ++k) sgd_element(wv.v[k], gv.v[k], av.v[k], nb[k] & 1, lr, mom, l2, gs);
        vstore<VEC>(w + e0, wv);
        vstore<VEC>(acc + e0, av);
    } else {
#pragma unroll
        for (int k = 0; k < VEC; ++k)
            if (e0 + k < n) {
                float wv = w[e0 + k], av = acc[e0 + k];
                sgd_element(wv, g[e0 + k], av, nb[k] & 1, lr, mom, l2, gs);
                w[e0 + k] = wv;
                acc[e0 + k] = av;
            }
    }
}

bool overlap(const void* a, const void* b, int64_t bytes)
{
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + (uintptr_t)bytes && y < x + (uintptr_t)bytes;
}

// ---- the graph walker --------------------------------------------------------------------------------------------------------------------------

struct Rec {  // what a layer's backward needs of its forward
    const float *in, *in2;
    int l, C1, C2, up, stride, dil;
};

struct Step {
    ps_context* c;
    bool run;
    Net net;
    StepPlan p;
    char* base;
    const float* wt;
    float* gr;
    int prec_fwd, prec_data, prec_weight;  // PS_PREC_*: the convolutions of each role
    size_t ops_need = 0;
    Rec rec[48];

    float* at(size_t off) const { return base ? reinterpret_cast<float*>(base + off) : nullptr; }
    float* X(int li) const { return at(p.X[li]); }
    float* Y(int li) const { return at(p.Y[li]); }
    size_t rows(int l) const { return (size_t)p.B * p.Vl[l]; }

    // an op with scratch: f(scratch, &bytes).  Off: the size alone (and the op's own argument checks); on: the plan's op region.
    template <class F>
    int op(F f)
    {
        int64_t n = 0;
        if (!run) {
            PS_TRY(f(nullptr, &n));
            ops_need = std::max(ops_need, (size_t)n);
            return PS_OK;
        }
        n = (int64_t)p.ops_bytes;
        return f(base + p.ops, &n);
    }

    void cols(const float* a, int lda, const float* b, int ldb, int l, int C, float* dst, int ldd)
    {
        if (!run) return;
        Stage stg(c, "saliency_step_cols", 1);
        cols_run(c->stream, a, lda, b, ldb, rows(l), C, dst, ldd);
    }

    // one layer: the convolution of `in` ([B, level l's extents, C1]; in2: the C2 channels behind it; both up-sampled `up` times) into X,
    // its norm + ReLU into Y
    int fwd(int li, const float* in, const float* in2, int l, int C2, int up, int stride, int dil, float* x_over = nullptr)
    {
        const Layer& L = net.L[li];
        rec[li] = {in, in2, l, L.cin - C2, C2, up, stride, dil};
        float* x = x_over ? x_over : X(li);
        if (run)
            PS_TRY(ps_conv3d_prec(c, in, in2, p.B, p.Dl[l], p.Hl[l], p.Wl[l], L.cin - C2, C2, up, wt + L.w, L.b >= 0 ? wt + L.b : nullptr, L.kd, L.kh, L.kw,
                                  L.cout, stride, dil, x, prec_fwd));
        if (L.g < 0) return PS_OK;
        const int lo = p.level[li];
        return op([&](void* sc, int64_t* n) {
            return ps_instance_norm_relu(c, x, p.B, p.Vl[lo], L.cout, wt + L.g, wt + L.be, 1e-5f, Y(li), sc, n);
        });
    }

    // its backward: dy, the gradient of Y -> (through the norm, into dxn, which may be dy) the gradient of X -> the layer's parameters'
    // gradients at their offsets in `grads`, and -- with `data` -- the input's gradient into dx / dx2 (dense; dx2 NULL without a second input)
    int bwd(int li, const float* dy, float* dxn, float* dx, float* dx2, bool data = true)
    {
        const Layer& L = net.L[li];
        const Rec& r = rec[li];
        const int lo = p.level[li];
        const float* g = dy;
        if (L.g >= 0) {
            PS_TRY(op([&](void* sc, int64_t* n) {
                return ps_instance_norm_relu_bwd(c, X(li), Y(li), dy, p.B, p.Vl[lo], L.cout, wt + L.g, 1e-5f, dxn, gr + L.g, gr + L.be, sc, n);
            }));
            g = dxn;
        }
        PS_TRY(op([&](void* sc, int64_t* n) {
            return ps_conv3d_bwd_weight_prec(c, r.in, r.in2, g, p.B, p.Dl[r.l], p.Hl[r.l], p.Wl[r.l], r.C1, r.C2, r.up, L.kd, L.kh, L.kw, L.cout, r.stride,
                                             r.dil, gr + L.w, L.b >= 0 ? gr + L.b : nullptr, sc, n, prec_weight);
        }));
        if (!data) return PS_OK;
        return op([&](void* sc, int64_t* n) {
            return ps_conv3d_bwd_data_prec(c, g, wt + L.w, p.B, p.Dl[r.l], p.Hl[r.l], p.Wl[r.l], r.C1, r.C2, r.up, L.kd, L.kh, L.kw, L.cout, r.stride, r.dil, dx,
                                           dx2, sc, n, prec_data);
        });
    }

    // the four branches of a CFE3D on down_list[2 + q]: their gradients out of `src` (pitch ld) into the gradient of down_list[2 + q],
    // the last branch written, the others added
    int cfe_bwd(int q, const float* src, int ld, float* gb)
    {
        const int l = 2 + q;
        for (int r = 3; r >= 0; --r) {
            cols(src ? src + 32 * r : nullptr, ld, nullptr, 0, l, 32, gb, 32);
            float* to = r == 3 ? at(p.gdn[l]) : at(p.tA[l]);
            PS_TRY(bwd(net.cfe[q][r], gb, gb, to, nullptr));
            if (r < 3) cols(at(p.gdn[l]), 16 << l, to, 16 << l, l, 16 << l, at(p.gdn[l]), 16 << l);
        }
        return PS_OK;
    }

    // labels: [B, D, H, W] int32, or -- soft -- the f32 [B, D, H, W, K] rows of include/pointseg_saliency_mixup.h: the loss node's kind
    int walk(const float* x, const void* labels, bool soft, const float* weight, float* loss, float* logits_out)
    {
        const int nB = p.B, K = p.K, V0 = p.Vl[0];
        // ---- forward: the encoder (model.py:182-210)
        PS_TRY(fwd(net.init, x, nullptr, 0, 0, 1, 1, 1));
        const float* cur = Y(net.init);
        float* dn[5];
        for (int d = 0; d < 5; ++d) {
            const int w = 16 << d;
            PS_TRY(fwd(net.down[d][0], cur, nullptr, d, 0, 1, 1, 1));
            PS_TRY(fwd(net.down[d][1], Y(net.down[d][0]), nullptr, d, 0, 1, 1, 1));
            dn[d] = at(p.dn[d]);
            cols(cur, w, Y(net.down[d][1]), w, d, w, dn[d], w);  // the residual add
            if (d < 4) {
                PS_TRY(fwd(net.s2[d], dn[d], nullptr, d, 0, 1, 2, 1));
                cur = Y(net.s2[d]);
            }
        }
        // the low-level features (model.py:212-228)
        PS_TRY(fwd(net.c1, dn[0], nullptr, 0, 0, 1, 1, 1));
        PS_TRY(fwd(net.c2, dn[1], nullptr, 1, 0, 1, 1, 1));
        // the high-level features: CFE3D on down_list[2..4], the deeper two up-sampled to level 2 (model.py:239-251)
        float* cat345 = at(p.cat345);
        float* cfe_out[3] = {cat345, at(p.cfecat[1]), at(p.cfecat[2])};
        const int cfe_ld[3] = {kCA, 128, 128}, rate[4] = {1, 3, 5, 7};
        for (int q = 0; q < 3; ++q)
            for (int r = 0; r < 4; ++r) {
                PS_TRY(fwd(net.cfe[q][r], dn[2 + q], nullptr, 2 + q, 0, 1, 1, rate[r]));
                cols(Y(net.cfe[q][r]), 32, nullptr, 0, 2 + q, 32, cfe_out[q] ? cfe_out[q] + 32 * r : nullptr, cfe_ld[q]);
            }
        PS_TRY(fwd(net.up4, cfe_out[1], nullptr, 3, 0, 2, 1, 1));
        cols(Y(net.up4), 128, nullptr, 0, 2, 128, cat345 ? cat345 + 128 : nullptr, kCA);
        PS_TRY(fwd(net.up5, cfe_out[2], nullptr, 4, 0, 4, 1, 1));
        cols(Y(net.up5), 128, nullptr, 0, 2, 128, cat345 ? cat345 + 256 : nullptr, kCA);
        // the channel attention, applied to the tensor; C345_conv; up to full resolution (model.py:255-271)
        const Layer &d1 = net.L[net.d1], &d2 = net.L[net.d2];
        float *mean = at(p.mean), *hidden = at(p.hidden), *scale = at(p.scale), *ca_y = at(p.ca_y);
        PS_TRY(op([&](void* sc, int64_t* n) {
            return ps_channel_attention(c, cat345, nB, p.Vl[2], kCA, kCAh, wt + d1.w, wt + d1.b, wt + d2.w, wt + d2.b, mean, hidden, scale, ca_y, sc, n);
        }));
        PS_TRY(fwd(net.c345, ca_y, nullptr, 2, 0, 1, 1, 1));
        PS_TRY(fwd(net.up345, Y(net.c345), nullptr, 2, 0, 4, 1, 1));
        const float* c345u = Y(net.up345);
        // the spatial attention (attention.py:79-154)
        for (int i = 0; i < 3; ++i) {
            PS_TRY(fwd(net.sa[i][0], c345u, nullptr, 0, 0, 1, 1, 1));
            PS_TRY(fwd(net.sa[i][1], Y(net.sa[i][0]), nullptr, 0, 0, 1, 1, 1));
        }
        // C12 and the gate (model.py:278-295)
        PS_TRY(fwd(net.upc2, Y(net.c2), nullptr, 1, 0, 2, 1, 1));
        PS_TRY(fwd(net.c12, Y(net.c1), Y(net.upc2), 0, 64, 1, 1, 1));
        float *sa_map = at(p.sa_map), *gated = at(p.gated);
        if (run) PS_TRY(ps_spatial_gate(c, Y(net.sa[0][1]), Y(net.sa[1][1]), Y(net.sa[2][1]), Y(net.c12), nB, V0, 64, sa_map, gated));
        // the logits and the loss (model.py:298-307, 491-548, 592-618)
        float* lg = logits_out ? logits_out : at(p.logits);
        PS_TRY(fwd(net.fin, gated, c345u, 0, 64, 1, 1, 1, lg));
        double* sums = reinterpret_cast<double*>(at(p.sums));
        PS_TRY(op([&](void* sc, int64_t* n) {
            return (soft ? ps_softmax_dice_soft_loss : ps_softmax_dice_loss)(c, lg, labels, weight, nB, V0, K, loss, sums, sc, n);
        }));

        // ---- backward, the readers of a shared tensor in the reverse of the header's layer order
        float *gK = at(p.gK), *gA = at(p.gA), *gB = at(p.gB), *gC = at(p.gC), *gD = at(p.gD), *gS = at(p.gS), *g1 = at(p.g1), *g1b = at(p.g1b);
        float *gdn[5], *tA[5], *tB[5];
        for (int l = 0; l < 5; ++l) gdn[l] = at(p.gdn[l]), tA[l] = at(p.tA[l]), tB[l] = at(p.tB[l]);
        if (run) PS_TRY((soft ? ps_softmax_dice_soft_loss_bwd : ps_softmax_dice_loss_bwd)(c, lg, labels, weight, sums, nullptr, nB, V0, K, gK));
        PS_TRY(bwd(net.fin, gK, nullptr, gA, gB));  // gA: the gated C12's gradient; gB: C345's, the first of its four
        if (run) PS_TRY(ps_spatial_gate_bwd(c, gA, Y(net.c12), sa_map, nB, V0, 64, gA, g1));
        PS_TRY(bwd(net.c12, gA, gA, gC, gD));
        PS_TRY(bwd(net.upc2, gD, gD, at(p.g1c2), nullptr));
        PS_TRY(bwd(net.c1, gC, gC, gdn[0], nullptr));
        for (int i = 2; i >= 0; --i) {
            PS_TRY(bwd(net.sa[i][1], g1, g1b, gS, nullptr));  // (g1 is every branch's: the norm's gradient goes to g1b)
            PS_TRY(bwd(net.sa[i][0], gS, gS, gA, nullptr));
            cols(gB, 64, gA, 64, 0, 64, gB, 64);
        }
        float *g2c = at(p.g2c), *g2cat = at(p.g2cat), *g2p = at(p.g2p);
        PS_TRY(bwd(net.up345, gB, gB, g2c, nullptr));
        PS_TRY(bwd(net.c345, g2c, g2c, g2cat, nullptr));
        PS_TRY(op([&](void* sc, int64_t* n) {
            return ps_channel_attention_bwd(c, cat345, g2cat, mean, hidden, scale, wt + d1.w, wt + d2.w, nB, p.Vl[2], kCA, kCAh, g2cat, gr + d1.w, gr + d1.b,
                                            gr + d2.w, gr + d2.b, sc, n);
        }));
        cols(g2cat ? g2cat + 256 : nullptr, kCA, nullptr, 0, 2, 128, g2p, 128);
        PS_TRY(bwd(net.up5, g2p, g2p, at(p.g4cfe), nullptr));
        PS_TRY(cfe_bwd(2, at(p.g4cfe), 128, at(p.g4b)));
        cols(g2cat ? g2cat + 128 : nullptr, kCA, nullptr, 0, 2, 128, g2p, 128);
        PS_TRY(bwd(net.up4, g2p, g2p, at(p.g3cfe), nullptr));
        PS_TRY(cfe_bwd(1, at(p.g3cfe), 128, at(p.g3b)));
        PS_TRY(cfe_bwd(0, g2cat, kCA, at(p.g2b)));
        PS_TRY(bwd(net.c2, at(p.g1c2), at(p.g1c2), gdn[1], nullptr));
        // the encoder, bottom up: gdn[d] is down_list[d]'s gradient, then the block's input's
        for (int d = 4; d >= 0; --d) {
            const int w = 16 << d;
            PS_TRY(bwd(net.down[d][1], gdn[d], tA[d], tB[d], nullptr));
            PS_TRY(bwd(net.down[d][0], tB[d], tB[d], tA[d], nullptr));
            cols(gdn[d], w, tA[d], w, d, w, gdn[d], w);
            if (d > 0) {
                PS_TRY(bwd(net.s2[d - 1], gdn[d], gdn[d], tA[d - 1], nullptr));
                cols(gdn[d - 1], w / 2, tA[d - 1], w / 2, d - 1, w / 2, gdn[d - 1], w / 2);
            } else {
                PS_TRY(bwd(net.init, gdn[0], gdn[0], nullptr, nullptr, false));  // (the patch wants no gradient)
            }
        }
        if (run) PS_HIP(hipGetLastError());
        return PS_OK;
    }
};

int shapes_ok(const char* who, int64_t B, int64_t D, int64_t H, int64_t W, int64_t C_in, int64_t K)
{
    PS_CHECK(net_args_ok(C_in, K), "%s: C_in = %lld, num_classes = %lld (1 <= C_in <= 16, 2 <= num_classes <= 16)", who, (long long)C_in, (long long)K);
    PS_CHECK(B >= 1 && B <= 1024, "%s: B = %lld, must be in [1, 1024]", who, (long long)B);
    PS_CHECK(D >= 16 && H >= 16 && W >= 16 && D % 16 == 0 && H % 16 == 0 && W % 16 == 0,
             "%s: patch %lld x %lld x %lld, every extent must be a positive multiple of 16 (four stride-2 levels)", who, (long long)D, (long long)H, (long long)W);
    PS_CHECK(D < (1 << 20) && H < (1 << 20) && W < (1 << 20) && D * H < (1ll << 31) && D * H * W < (1ll << 31) && B * D * H * W * 128 < (1ll << 31),
             "%s: patch %lld x %lld x %lld, B * D * H * W * 128 must stay below 2^31", who, (long long)D, (long long)H, (long long)W);
    return PS_OK;
}

// soft_labels and the three precisions of include/pointseg_saliency_step_precision.h, as the caller gave them
struct Modes {
    int32_t soft, fwd, data, weight;
};

const Modes kFp32Hard = {0, PS_PREC_FP32, PS_PREC_FP32, PS_PREC_FP32}, kFp32Soft = {1, PS_PREC_FP32, PS_PREC_FP32, PS_PREC_FP32};

int modes_ok(const char* who, const Modes& m)
{
    PS_CHECK(m.soft == 0 || m.soft == 1, "%s: soft_labels = %d, must be 0 (int32 labels) or 1 (float32 rows)", who, (int)m.soft);
    PS_CHECK(precision_ok(m.fwd) && precision_ok(m.data) && precision_ok(m.weight),
             "%s: precision_forward = %d, precision_data_grad = %d, precision_weight_grad = %d, each must be PS_PREC_FP32 (0), PS_PREC_BF16X3 (1) or "
             "PS_PREC_BF16 (2)",
             who, (int)m.fwd, (int)m.data, (int)m.weight);
    return PS_OK;
}

// ps_saliency_backward_prec behind checked shapes; `who` names the entry in the messages
int backward_run(const char* who, const Modes& m, ps_context* c, const void* x, const void* labels, const void* weight, int64_t B, int64_t D, int64_t H, int64_t W, int64_t C_in,
                 int64_t K, const void* weights, int64_t weight_count, void* grads, void* loss, void* logits, void* scratch, int64_t* scratch_bytes)
{
    PS_TRY(modes_ok(who, m));
    PS_CHECK(scratch_bytes && (c || !scratch), "%s: NULL argument", who);
    PS_TRY(shapes_ok(who, B, D, H, W, C_in, K));
    const bool soft = m.soft != 0;
    Step s;
    s.prec_fwd = m.fwd, s.prec_data = m.data, s.prec_weight = m.weight;
    build_net(s.net, (int)C_in, (int)K);
    PS_CHECK(weight_count == s.net.count, "%s: weight_count = %lld, the network has %lld weights", who, (long long)weight_count, (long long)s.net.count);
    s.c = c, s.run = false, s.base = nullptr, s.wt = nullptr, s.gr = nullptr;
    step_plan(s.net, (int)B, (int)D, (int)H, (int)W, (int)K, 0, s.p);
    PS_TRY(s.walk(nullptr, nullptr, soft, nullptr, nullptr, nullptr));  // every op's size, and its own view of the shapes
    step_plan(s.net, (int)B, (int)D, (int)H, (int)W, (int)K, s.ops_need, s.p);
    if (!scratch) {
        *scratch_bytes = (int64_t)s.p.total;
        return PS_OK;
    }
    PS_CHECK(x && labels && weights && grads && loss,
             "%s: NULL x, labels, weights, grads or loss (they may be NULL only in the call that sizes the scratch; weight and logits may be NULL)", who);
    PS_CHECK(!overlap(weights, grads, weight_count * 4), "%s: grads must not overlap weights", who);
    PS_TRY(check_scratch(who, scratch, scratch_bytes, s.p.total));
    PS_HIP(hipSetDevice(c->device));
    s.run = true, s.base = static_cast<char*>(scratch), s.wt = static_cast<const float*>(weights), s.gr = static_cast<float*>(grads);
    return s.walk(static_cast<const float*>(x), labels, soft, static_cast<const float*>(weight), static_cast<float*>(loss), static_cast<float*>(logits));
}

int update_check(const char* who, const void* params, const void* grads, const void* accum, int64_t C_in, int64_t K, int64_t weight_count, Net& net)
{
    PS_CHECK(net_args_ok(C_in, K), "%s: C_in = %lld, num_classes = %lld (1 <= C_in <= 16, 2 <= num_classes <= 16)", who, (long long)C_in, (long long)K);
    build_net(net, (int)C_in, (int)K);
    PS_CHECK(weight_count == net.count, "%s: weight_count = %lld, the network has %lld weights", who, (long long)weight_count, (long long)net.count);
    PS_CHECK(params && grads && accum, "%s: NULL params, grads or accum", who);
    PS_CHECK(!overlap(params, grads, weight_count * 4) && !overlap(params, accum, weight_count * 4) && !overlap(grads, accum, weight_count * 4),
             "%s: params, grads and accum must not overlap", who);
    return PS_OK;
}

void update_run(hipStream_t sm, const Net& net, float* params, const float* grads, float* accum, float lr, float momentum, float l2, float grad_scale)
{
    DecayTable t;
    decay_table(net, t);
    const int n = (int)net.count;
    if (aligned16(params) && aligned16(grads) && aligned16(accum))
        hipLaunchKernelGGL(sgd_update_kernel<4>, dim3(blocks256((size_t)(n + 3) / 4)), dim3(256), 0, sm, params, grads, accum, n, t, lr, momentum, l2, grad_scale);
    else
        hipLaunchKernelGGL(sgd_update_kernel<1>, dim3(blocks256((size_t)n)), dim3(256), 0, sm, params, grads, accum, n, t, lr, momentum, l2, grad_scale);
}

}  // namespace

}  // namespace ps

extern "C" int ps_saliency_backward(ps_context* c, const void* x, const void* labels, const void* weight, int64_t B, int64_t D, int64_t H, int64_t W,
                                    int64_t C_in, int64_t num_classes, const void* weights, int64_t weight_count, void* grads, void* loss, void* logits,
                                    void* scratch, int64_t* scratch_bytes)
{
    return ps::backward_run("ps_saliency_backward", ps::kFp32Hard, c, x, labels, weight, B, D, H, W, C_in, num_classes, weights, weight_count, grads, loss, logits, scratch,
                            scratch_bytes);
}

extern "C" int ps_saliency_sgd_update(ps_context* c, void* params, const void* grads, void* accum, int64_t C_in, int64_t num_classes, int64_t weight_count,
                                      float learning_rate, float momentum, float l2, float grad_scale)
{
    using namespace ps;
    static const char* who = "ps_saliency_sgd_update";
    Net net;
    PS_TRY(update_check(who, params, grads, accum, C_in, num_classes, weight_count, net));
    PS_CHECK(c, "%s: NULL context", who);
    PS_HIP(hipSetDevice(c->device));
    Stage stg(c, "saliency_sgd_update", 1);
    update_run(c->stream, net, static_cast<float*>(params), static_cast<const float*>(grads), static_cast<float*>(accum), learning_rate, momentum, l2, grad_scale);
    PS_HIP(hipGetLastError());
    return PS_OK;
}

namespace ps {

namespace {

// ps_saliency_train_step_prec
int train_step_run(const char* who, const Modes& m, ps_context* c, const void* x, const void* labels, const void* weight, int64_t B, int64_t D, int64_t H, int64_t W,
                   int64_t C_in, int64_t num_classes, void* params, int64_t weight_count, void* grads, void* accum, float learning_rate,
                   const ps_saliency_step_options* options, void* loss, void* logits, void* scratch, int64_t* scratch_bytes)
{
    PS_TRY(modes_ok(who, m));
    const ps_saliency_step_options dflt = {nullptr, nullptr, 1, 0.9f, 1e-5f};
    const ps_saliency_step_options& o = options ? *options : dflt;
    PS_CHECK(o.world_size >= 1, "%s: world_size = %d, must be >= 1", who, (int)o.world_size);
    PS_CHECK(o.allreduce || o.world_size == 1, "%s: a world of %d ranks needs an all-reduce callback", who, (int)o.world_size);
    if (scratch) {  // (the sizing call looks at the shapes alone)
        Net net;
        PS_TRY(update_check(who, params, grads, accum, C_in, num_classes, weight_count, net));
    }
    PS_TRY(backward_run(who, m, c, x, labels, weight, B, D, H, W, C_in, num_classes, params, weight_count, grads, loss, logits, scratch, scratch_bytes));
    if (!scratch) return PS_OK;
    float grad_scale = 1.f;
    if (o.allreduce && o.world_size > 1) {
        const int rc = o.allreduce(o.user, grads, weight_count, 0, (void*)c->stream);
        if (rc != 0) {
            set_error("%s: the host's all-reduce callback failed with code %d", who, rc);
            return PS_ESTATE;
        }
        grad_scale = 1.f / (float)o.world_size;
    }
    Net net;
    build_net(net, (int)C_in, (int)num_classes);
    Stage stg(c, "saliency_sgd_update", 1);
    update_run(c->stream, net, static_cast<float*>(params), static_cast<const float*>(grads), static_cast<float*>(accum), learning_rate, o.momentum, o.l2, grad_scale);
    PS_HIP(hipGetLastError());
    return PS_OK;
}

}  // namespace

}  // namespace ps

extern "C" int ps_saliency_train_step(ps_context* c, const void* x, const void* labels, const void* weight, int64_t B, int64_t D, int64_t H, int64_t W,
                                      int64_t C_in, int64_t num_classes, void* params, int64_t weight_count, void* grads, void* accum, float learning_rate,
                                      const ps_saliency_step_options* options, void* loss, void* logits, void* scratch, int64_t* scratch_bytes)
{
    return ps::train_step_run("ps_saliency_train_step", ps::kFp32Hard, c, x, labels, weight, B, D, H, W, C_in, num_classes, params, weight_count, grads, accum,
                              learning_rate, options, loss, logits, scratch, scratch_bytes);
}

extern "C" int ps_saliency_backward_soft(ps_context* c, const void* x, const void* soft, const void* weight, int64_t B, int64_t D, int64_t H, int64_t W,
                                         int64_t C_in, int64_t num_classes, const void* weights, int64_t weight_count, void* grads, void* loss, void* logits,
                                         void* scratch, int64_t* scratch_bytes)
{
    return ps::backward_run("ps_saliency_backward_soft", ps::kFp32Soft, c, x, soft, weight, B, D, H, W, C_in, num_classes, weights, weight_count, grads, loss, logits,
                            scratch, scratch_bytes);
}

extern "C" int ps_saliency_train_step_soft(ps_context* c, const void* x, const void* soft, const void* weight, int64_t B, int64_t D, int64_t H, int64_t W,
                                           int64_t C_in, int64_t num_classes, void* params, int64_t weight_count, void* grads, void* accum, float learning_rate,
                                           const ps_saliency_step_options* options, void* loss, void* logits, void* scratch, int64_t* scratch_bytes)
{
    return ps::train_step_run("ps_saliency_train_step_soft", ps::kFp32Soft, c, x, soft, weight, B, D, H, W, C_in, num_classes, params, weight_count, grads, accum,
                              learning_rate, options, loss, logits, scratch, scratch_bytes);
}

extern "C" int ps_saliency_backward_prec(ps_context* c, const void* x, const void* labels, const void* weight, int64_t B, int64_t D, int64_t H, int64_t W,
                                         int64_t C_in, int64_t num_classes, const void* weights, int64_t weight_count, void* grads, void* loss, void* logits,
                                         void* scratch, int64_t* scratch_bytes, int32_t soft_labels, int32_t precision_forward, int32_t precision_data_grad,
                                         int32_t precision_weight_grad)
{
    const ps::Modes m = {soft_labels, precision_forward, precision_data_grad, precision_weight_grad};
    return ps::backward_run("ps_saliency_backward_prec", m, c, x, labels, weight, B, D, H, W, C_in, num_classes, weights, weight_count, grads, loss, logits, scratch,
                            scratch_bytes);
}

extern "C" int ps_saliency_train_step_prec(ps_context* c, const void* x, const void* labels, const void* weight, int64_t B, int64_t D, int64_t H, int64_t W,
                                           int64_t C_in, int64_t num_classes, void* params, int64_t weight_count, void* grads, void* accum, float learning_rate,
                                           const ps_saliency_step_options* options, void* loss, void* logits, void* scratch, int64_t* scratch_bytes,
                                           int32_t soft_labels, int32_t precision_forward, int32_t precision_data_grad, int32_t precision_weight_grad)
{
    const ps::Modes m = {soft_labels, precision_forward, precision_data_grad, precision_weight_grad};
    return ps::train_step_run("ps_saliency_train_step_prec", m, c, x, labels, weight, B, D, H, W, C_in, num_classes, params, weight_count, grads, accum,
                              learning_rate, options, loss, logits, scratch, scratch_bytes);
}
