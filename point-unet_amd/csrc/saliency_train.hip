// saliency_train.hip -- the gradients of saliency.hip's ops: instance norm + ReLU (include/pointseg_saliency_train.h), and the
// channel attention, the spatial gate and softmax + weighted Dice, each with the forward a training step records
// (include/pointseg_saliency_attention.h).  The convolution's gradients are conv3d_train.hip's.  What these ops share with
// saliency.hip's fused forward -- the slab sums, the moments, the channel attention's dense part, the gate, the softmax -- is saliency_kit.h's.
//
// All of them are memory-bound: a pass reads or writes each large tensor once, 16 bytes per lane along the channel axis where C % 4 == 0
// and the tensors are 16-byte aligned (VEC = 4), a float at a time elsewhere (VEC = 1) -- the same values either way, a lane adds its own
// channels only.  Every sum over voxels goes through the kit's slab-sum frame (the loss keeps its own wave-butterfly form).
#include "../../include/pointseg_saliency_attention.h"
#include "../../include/pointseg_saliency_mixup.h"
#include "../../include/pointseg_saliency_train.h"
#include "dice_kit.h"
#include "saliency_kit.h"

namespace ps {

namespace {

constexpr int kMaxC = 1024, kMaxCh = 256;

// ---- instance norm + ReLU ------------------------------------------------------------------------------------------------------------------------

// (sum g, sum g xhat) with g = dy where y > 0 and xhat = (x - mean) * rstd from stat[b * C + c]
struct NormBwdSums {
    static constexpr int kUnroll = 4;
    const float* __restrict__ x;
    const float* __restrict__ y;
    const float* __restrict__ dy;
    const double2* __restrict__ stat;
    __device__ __forceinline__ void operator()(int bc, size_t e, double (&d)[2]) const
    {
        const double2 st = stat[bc];
        const double f = (double)x[e], g = y[e] > 0.f ? (double)dy[e] : 0.0;
        d[0] = g;
        d[1] = g * ((f - st.x) * st.y);
    }
};

// tot[(b * C + c) * 2 + {0, 1}] -> stat[b * C + c] = (mean, 1 / sqrt(var + eps))
__global__ __launch_bounds__(256) void in_bwd_stat_kernel(const double* __restrict__ tot, int V, int BC, float eps, double2* __restrict__ stat)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= BC) return;
    const double2 m = moments(tot, i, V, eps);
    stat[i] = make_double2(m.x, 1.0 / m.y);
}

// grid (ceil(V * C / 256), B): dx = gamma * rstd * (g - mean(g) - xhat * mean(g xhat)); every element reads its own dy before it writes dx
__global__ __launch_bounds__(256) void in_bwd_dx_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* dy, int V, int C,
                                                        const double2* __restrict__ stat, const double* __restrict__ tot2, const float* __restrict__ gamma,
                                                        float* dx)
{
    const unsigned e = blockIdx.x * 256u + threadIdx.x;
    if (e >= (unsigned)V * (unsigned)C) return;
    const unsigned c = e % (unsigned)C;
    const size_t i = (size_t)blockIdx.y * V * C + e;
    const int bc = blockIdx.y * C + c;
    const double2 st = stat[bc];
    const double mg = tot2[2 * bc] / V, mgx = tot2[2 * bc + 1] / V;
    const double g = y[i] > 0.f ? (double)dy[i] : 0.0;
    const double xh = ((double)x[i] - st.x) * st.y;
    dx[i] = (float)((double)gamma[c] * st.y * (g - mg - xh * mgx));
}

// dbeta[c] = sum over b of tot2[b][c][0], dgamma[c] = sum over b of tot2[b][c][1], b ascending
__global__ __launch_bounds__(256) void in_bwd_params_kernel(const double* __restrict__ tot2, int B, int C, float* __restrict__ dgamma, float* __restrict__ dbeta)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double sb = 0.0, sg = 0.0;
    for (int b = 0; b < B; ++b) {
        sb += tot2[((size_t)b * C + c) * 2];
        sg += tot2[((size_t)b * C + c) * 2 + 1];
    }
    if (dbeta) dbeta[c] = (float)sb;
    if (dgamma) dgamma[c] = (float)sg;
}

// ---- channel attention -------------------------------------------------------------------------------------------------------------------------

// part [slabs][B][C] and tot [B][C]: tot[b, c] = sum over v of a[b, v, c] (* m[b, v, c])
void colsum_run(hipStream_t sm, const float* a, const float* m, int B, int V, int C, double* part, double* tot)
{
    if (C % 4 == 0 && aligned16(a) && aligned16(m)) {
        if (m) slab_sum_run<4, 1>(sm, ColumnSum<4, true>{a, m}, C, B, V, C, part, tot);
        else slab_sum_run<4, 1>(sm, ColumnSum<4, false>{a, m}, C, B, V, C, part, tot);
    } else {
        if (m) slab_sum_run<1, 1>(sm, ColumnSum<1, true>{a, m}, C, B, V, C, part, tot);
        else slab_sum_run<1, 1>(sm, ColumnSum<1, false>{a, m}, C, B, V, C, part, tot);
    }
}

// One workgroup per sample: the kit's dense part, the three vectors kept for the gradient.
__global__ __launch_bounds__(256) void ca_dense_kernel(const double* __restrict__ tot, int V, int C, int Ch, const float* __restrict__ w1,
                                                       const float* __restrict__ b1, const float* __restrict__ w2, const float* __restrict__ b2,
                                                       float* __restrict__ mean_out, float* __restrict__ hidden_out, float* __restrict__ scale_out)
{
    __shared__ float mean[kMaxC], h[kMaxCh], s[kMaxC];
    const int t = threadIdx.x, b = blockIdx.x;
    ca_dense(tot + (size_t)b * C, 1, V, C, Ch, w1, b1, w2, b2, mean, h, s);
    for (int c = t; c < C; c += 256) {
        mean_out[(size_t)b * C + c] = mean[c];
        scale_out[(size_t)b * C + c] = s[c];
    }
    for (int i = t; i < Ch; i += 256) hidden_out[(size_t)b * Ch + i] = h[i];
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

// ---- softmax + weighted Dice: the kernels of dice_kit.h behind a softmax and a per-voxel weight map --------------------------------------------

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


// the vector MODE all of a call's rows can be moved in: the logits (read at a, written at b) and, soft labels, their rows
inline int dice_mode_with(int C, const void* a, const void* b, const SoftLabels& l)
{
    const int m = dice_mode(C, a, b);
    return dice_mode(C, l.p, l.p) == m ? m : 1;
}
inline int dice_mode_with(int C, const void* a, const void* b, const HardLabels&) { return dice_mode(C, a, b); }

// ps_softmax_dice_loss / ps_softmax_dice_soft_loss behind one body; `what` names the label argument in the messages
template <class LAB>
int dice_loss_run(const char* who, const char* what, ps_context* c, const void* logits, LAB labels, const void* weight, int64_t B, int64_t V, int64_t C,
                  void* loss, void* sums, void* scratch, int64_t* scratch_bytes)
{
    PS_CHECK(scratch_bytes, "%s: NULL scratch_bytes", who);
    PS_TRY(rows_shape_ok(who, B, V, C, 2, kMaxClasses, kLimitV));
    const int slabs = ceil_div(V, kSlab), nv = (int)(B * C * 3);
    Carver cv{static_cast<char*>(scratch)};
    double* part = cv.take<double>((size_t)slabs * nv);
    if (!scratch) {
        *scratch_bytes = (int64_t)cv.off;
        return PS_OK;
    }
    PS_CHECK(logits && labels.p, "%s: NULL logits or %s (they may be NULL only in the call that sizes the scratch; weight may be NULL)", who, what);
    PS_CHECK(loss && sums, "%s: NULL loss or sums", who);
    PS_CHECK(c, "%s: NULL context", who);
    PS_TRY(check_scratch(who, scratch, scratch_bytes, cv.off));

    PS_HIP(hipSetDevice(c->device));
    hipStream_t sm = c->stream;
    Stage stg(c, who + 3, 3);  // (the stage is the entry's name without "ps_")
    const float* lf = static_cast<const float*>(logits);
    const MapWeight wt{static_cast<const float*>(weight)};
    const dim3 grid((unsigned)slabs, (unsigned)B);
    const int mode = dice_mode_with((int)C, logits, logits, labels);
    if (mode == 2) hipLaunchKernelGGL((dice_sums_kernel<2, LAB, SoftmaxAct, MapWeight>), grid, dim3(256), 0, sm, lf, labels, wt, (int)V, (int)C, part);
    else if (mode == 4) hipLaunchKernelGGL((dice_sums_kernel<4, LAB, SoftmaxAct, MapWeight>), grid, dim3(256), 0, sm, lf, labels, wt, (int)V, (int)C, part);
    else hipLaunchKernelGGL((dice_sums_kernel<1, LAB, SoftmaxAct, MapWeight>), grid, dim3(256), 0, sm, lf, labels, wt, (int)V, (int)C, part);
    hipLaunchKernelGGL(reduce_partials_kernel<double>, dim3((unsigned)ceil_div(nv, 16)), dim3(256), 0, sm, part, slabs, nv, static_cast<double*>(sums));
    hipLaunchKernelGGL(dice_finish_kernel, dim3(1), dim3(64), 0, sm, static_cast<const double*>(sums), (int)B, (int)C, static_cast<float*>(loss));
    PS_HIP(hipGetLastError());
    return PS_OK;
}

template <class LAB>
int dice_bwd_run(const char* who, const char* what, ps_context* c, const void* logits, LAB labels, const void* weight, const void* sums, const void* dloss,
                 int64_t B, int64_t V, int64_t C, void* dlogits)
{
    PS_TRY(rows_shape_ok(who, B, V, C, 2, kMaxClasses, kLimitV));
    PS_CHECK(logits && labels.p && sums, "%s: NULL logits, %s or sums (weight and dloss may be NULL)", who, what);
    PS_CHECK(dlogits, "%s: NULL dlogits", who);
    PS_CHECK(c, "%s: NULL context", who);

    PS_HIP(hipSetDevice(c->device));
    Stage stg(c, who + 3, 1);
    const float* lf = static_cast<const float*>(logits);
    const MapWeight wt{static_cast<const float*>(weight)};
    const MapWeight::Finish fin{static_cast<const float*>(dloss)};
    const double* sd = static_cast<const double*>(sums);
    float* out = static_cast<float*>(dlogits);
    const dim3 grid((unsigned)ceil_div(V, 256), (unsigned)B);
    const int mode = dice_mode_with((int)C, logits, dlogits, labels);
    if (mode == 2) hipLaunchKernelGGL((dice_bwd_kernel<2, LAB, SoftmaxAct, MapWeight>), grid, dim3(256), 0, c->stream, lf, labels, wt, sd, fin, (int)B, (int)V, (int)C, out);
    else if (mode == 4) hipLaunchKernelGGL((dice_bwd_kernel<4, LAB, SoftmaxAct, MapWeight>), grid, dim3(256), 0, c->stream, lf, labels, wt, sd, fin, (int)B, (int)V, (int)C, out);
    else hipLaunchKernelGGL((dice_bwd_kernel<1, LAB, SoftmaxAct, MapWeight>), grid, dim3(256), 0, c->stream, lf, labels, wt, sd, fin, (int)B, (int)V, (int)C, out);
    PS_HIP(hipGetLastError());
    return PS_OK;
}

}  // namespace

}  // namespace ps

extern "C" int ps_instance_norm_relu_bwd(ps_context* c, const void* x, const void* y, const void* dy, int64_t B, int64_t V, int64_t C, const void* gamma, float eps,
                                         void* dx, void* dgamma, void* dbeta, void* scratch, int64_t* scratch_bytes)
{
    using namespace ps;
    static const char* who = "ps_instance_norm_relu_bwd";
    PS_CHECK(scratch_bytes, "%s: NULL scratch_bytes", who);
    PS_TRY(rows_shape_ok(who, B, V, C, 1, kMaxC, kLimitVC));
    PS_CHECK(eps > 0.f, "%s: eps = %g, must be > 0", who, (double)eps);
    const int slabs = ceil_div(V, kSlab), nv = (int)(B * C * 2);
    Carver cv{static_cast<char*>(scratch)};
    double* part = cv.take<double>((size_t)slabs * nv);
    double* tot = cv.take<double>((size_t)nv);
    double2* stat = cv.take<double2>((size_t)B * C);
    double* tot2 = cv.take<double>((size_t)nv);
    if (!scratch) {
        *scratch_bytes = (int64_t)cv.off;
        return PS_OK;
    }
    PS_CHECK(x && y && dy && gamma, "%s: NULL x, y, dy or gamma (they may be NULL only in the call that sizes the scratch)", who);
    PS_CHECK(dx || dgamma || dbeta, "%s: every result is NULL", who);
    PS_CHECK(dx != x && dx != y, "%s: dx must not overlap x or y (it may be dy)", who);
    PS_CHECK(c, "%s: NULL context", who);
    PS_TRY(check_scratch(who, scratch, scratch_bytes, cv.off));

    PS_HIP(hipSetDevice(c->device));
    hipStream_t sm = c->stream;
    Stage stg(c, "instance_norm_relu_bwd", 7);
    const float *xf = static_cast<const float*>(x), *yf = static_cast<const float*>(y), *dyf = static_cast<const float*>(dy);
    const int nB = (int)B, nV = (int)V, nC = (int)C;
    stats_run(sm, xf, nC, nB, nV, nC, part, tot);
    hipLaunchKernelGGL(in_bwd_stat_kernel, dim3(blocks256((size_t)nB * nC)), dim3(256), 0, sm, tot, nV, nB * nC, eps, stat);
    slab_sum_run<1, 2>(sm, NormBwdSums{xf, yf, dyf, stat}, nC, nB, nV, nC, part, tot2);
    if (dx)
        hipLaunchKernelGGL(in_bwd_dx_kernel, dim3(blocks256((size_t)nV * nC), (unsigned)nB), dim3(256), 0, sm, xf, yf, dyf, nV, nC, stat, tot2,
                           static_cast<const float*>(gamma), static_cast<float*>(dx));
    if (dgamma || dbeta)
        hipLaunchKernelGGL(in_bwd_params_kernel, dim3(blocks256((size_t)nC)), dim3(256), 0, sm, tot2, nB, nC, static_cast<float*>(dgamma),
                           static_cast<float*>(dbeta));
    PS_HIP(hipGetLastError());
    return PS_OK;
}

extern "C" int ps_channel_attention(ps_context* c, const void* x, int64_t B, int64_t V, int64_t C, int64_t Ch, const void* w1, const void* b1, const void* w2,
                                    const void* b2, void* mean, void* hidden, void* scale, void* y, void* scratch, int64_t* scratch_bytes)
{
    using namespace ps;
    static const char* who = "ps_channel_attention";
    PS_CHECK(scratch_bytes, "%s: NULL scratch_bytes", who);
    PS_TRY(rows_shape_ok(who, B, V, C, 1, kMaxC, kLimitVC));
    PS_CHECK(Ch >= 1 && Ch <= kMaxCh, "%s: Ch = %lld, must be in [1, %d]", who, (long long)Ch, kMaxCh);
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
    PS_TRY(rows_shape_ok(who, B, V, C, 1, kMaxC, kLimitVC));
    PS_CHECK(Ch >= 1 && Ch <= kMaxCh, "%s: Ch = %lld, must be in [1, %d]", who, (long long)Ch, kMaxCh);
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
    PS_TRY(rows_shape_ok(who, B, V, C, 1, kMaxC, kLimitBVC));
    PS_CHECK(a1 && a2 && a3 && f && sa && y, "%s: NULL a1, a2, a3, f, sa or y", who);
    PS_CHECK(c, "%s: NULL context", who);

    PS_HIP(hipSetDevice(c->device));
    Stage stg(c, "spatial_gate", 1);
    // dense rows: the B * V voxels as one sample
    PS_TRY(gate_run(c->stream, static_cast<const float*>(a1), static_cast<const float*>(a2), static_cast<const float*>(a3), static_cast<const float*>(f), (int)C,
                    1, (int)(B * V), (int)C, static_cast<float*>(sa), static_cast<float*>(y), (int)C));
    PS_HIP(hipGetLastError());
    return PS_OK;
}

extern "C" int ps_spatial_gate_bwd(ps_context* c, const void* dy, const void* f, const void* sa, int64_t B, int64_t V, int64_t C, void* df, void* da)
{
    using namespace ps;
    static const char* who = "ps_spatial_gate_bwd";
    PS_TRY(rows_shape_ok(who, B, V, C, 1, kMaxC, kLimitBVC));
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
    return ps::dice_loss_run("ps_softmax_dice_loss", "labels", c, logits, ps::HardLabels{static_cast<const int*>(labels)}, weight, B, V, C, loss, sums, scratch,
                             scratch_bytes);
}

extern "C" int ps_softmax_dice_loss_bwd(ps_context* c, const void* logits, const void* labels, const void* weight, const void* sums, const void* dloss, int64_t B,
                                        int64_t V, int64_t C, void* dlogits)
{
    return ps::dice_bwd_run("ps_softmax_dice_loss_bwd", "labels", c, logits, ps::HardLabels{static_cast<const int*>(labels)}, weight, sums, dloss, B, V, C,
                            dlogits);
}

extern "C" int ps_softmax_dice_soft_loss(ps_context* c, const void* logits, const void* soft, const void* weight, int64_t B, int64_t V, int64_t C, void* loss,
                                         void* sums, void* scratch, int64_t* scratch_bytes)
{
    return ps::dice_loss_run("ps_softmax_dice_soft_loss", "soft", c, logits, ps::SoftLabels{static_cast<const float*>(soft)}, weight, B, V, C, loss, sums,
                             scratch, scratch_bytes);
}

extern "C" int ps_softmax_dice_soft_loss_bwd(ps_context* c, const void* logits, const void* soft, const void* weight, const void* sums, const void* dloss,
                                             int64_t B, int64_t V, int64_t C, void* dlogits)
{
    return ps::dice_bwd_run("ps_softmax_dice_soft_loss_bwd", "soft", c, logits, ps::SoftLabels{static_cast<const float*>(soft)}, weight, sums, dloss, B, V, C,
                            dlogits);
}
