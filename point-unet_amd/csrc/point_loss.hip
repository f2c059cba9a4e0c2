// point_loss.hip -- the point network's Dice objectives (PointSegment/RandLANet.py:276-312) and the accuracy of its training step (:93-94) as
// ops (include/pointseg_train_loss.h).  The Dice is dice_kit.h's two kernels -- the ones behind the saliency network's loss
// -- with no activation in front (the reference takes it on the raw logits) and validity of the label as the row's weight, the class weight
// u_c entering at the finish.  ps_op_top1_counts is the same slab order around the accuracy rule alone, for the cross-entropy step.
//
// Memory-bound: the sums pass reads 4 C + 4 bytes per row, the from-sums pass reads them again and writes 4 C.  The partials live in the
// context's reduction workspace (red_ws), like ps_op_weighted_ce's.
#include <algorithm>

#include "../../include/pointseg_train_loss.h"
#include "dice_kit.h"

namespace ps {

namespace {

// rows of one launch: the kernels index a launch's rows in 32 bits (v + 256, v0 + kSlab and a grid's last thread stay below 2^31); a call
// of more rows is dealt in launches of whole slabs, whose partials line up behind one another -- the order of the additions is that of one launch
constexpr int64_t kRowsPerLaunch = 1ll << 30;

// n_valid, n_correct of the rows of a slab: the frame of dice_sums_kernel around row_top1's rule, for any C (the row is read from memory)
__global__ __launch_bounds__(256) void top1_counts_kernel(const float* __restrict__ logits, const int* __restrict__ labels, int V, int C,
                                                          double* __restrict__ part)
{
    __shared__ double red[4][2];
    const int t = threadIdx.x, v0 = blockIdx.x * kSlab, v1 = min(V, v0 + kSlab);
    double n0 = 0.0, n1 = 0.0;
    for (int v = v0 + t; v < v1; v += 256) {
        const int y = labels[v];
        if ((unsigned)y >= (unsigned)C) continue;
        const float* __restrict__ z = logits + (size_t)v * C;
        const float zt = z[y];
        bool ok = fabsf(zt) < INFINITY;
        for (int c = 0; c < C; ++c)
            if (z[c] > zt) ok = false;
        n0 += 1.0;
        if (ok) n1 += 1.0;
    }
    const double a0 = wave_sum(n0), a1 = wave_sum(n1);
    if ((t & 63) == 0) red[t >> 6][0] = a0, red[t >> 6][1] = a1;
    __syncthreads();
    if (t < 2) part[(size_t)blockIdx.x * 2 + t] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
}

int loss_shape_ok(const char* who, int64_t R, int64_t C, int64_t max_C)
{
    PS_CHECK(C >= 1 && C <= max_C, "%s: C = %lld, must be in [1, %lld]", who, (long long)C, (long long)max_C);
    PS_CHECK(R >= 1 && R < (1ll << 31), "%s: R = %lld, must be in [1, 2^31)", who, (long long)R);
    return PS_OK;
}

}  // namespace

}  // namespace ps

extern "C" int ps_op_dice_sums(ps_context* c, const float* logits, const int32_t* labels, int64_t R, int64_t C, double* sums)
{
    using namespace ps;
    static const char* who = "ps_op_dice_sums";
    PS_CHECK(c && logits && labels && sums, "%s: NULL argument", who);
    PS_TRY(loss_shape_ok(who, R, C, kMaxClasses));
    PS_HIP(hipSetDevice(c->device));
    const int slabs = ceil_div(R, kSlab), nv = (int)(3 * C + 2);
    PS_TRY(c->red_ws.reserve(sizeof(double) * (size_t)slabs * nv));
    double* part = c->red_ws.as<double>();
    Stage st(c, "train_loss", 2);
    const int mode = dice_mode((int)C, logits, logits);
    for (int64_t r0 = 0; r0 < R; r0 += kRowsPerLaunch) {
        const int V = (int)std::min(kRowsPerLaunch, R - r0);
        const dim3 grid((unsigned)ceil_div(V, kSlab), 1);
        const float* lf = logits + r0 * C;
        const HardLabels ll{labels + r0};
        double* pp = part + (r0 / kSlab) * nv;
        if (mode == 2) hipLaunchKernelGGL((dice_sums_kernel<2, HardLabels, NoAct, ValidWeight>), grid, dim3(256), 0, c->stream, lf, ll, ValidWeight{}, V, (int)C, pp);
        else if (mode == 4) hipLaunchKernelGGL((dice_sums_kernel<4, HardLabels, NoAct, ValidWeight>), grid, dim3(256), 0, c->stream, lf, ll, ValidWeight{}, V, (int)C, pp);
        else hipLaunchKernelGGL((dice_sums_kernel<1, HardLabels, NoAct, ValidWeight>), grid, dim3(256), 0, c->stream, lf, ll, ValidWeight{}, V, (int)C, pp);
    }
    hipLaunchKernelGGL(reduce_partials_kernel<double>, dim3((unsigned)ceil_div(nv, 16)), dim3(256), 0, c->stream, part, slabs, nv, sums);
    PS_HIP(hipGetLastError());
    return PS_OK;
}

extern "C" int ps_op_dice_from_sums(ps_context* c, int32_t kind, const float* logits, const int32_t* labels, const float* class_weights, const double* sums,
                                    float grad_scale, int64_t R, int64_t C, float* loss, float* dlogits)
{
    using namespace ps;
    static const char* who = "ps_op_dice_from_sums";
    PS_CHECK(kind == PS_LOSS_DICE || kind == PS_LOSS_DICE_WEIGHTED, "%s: kind = %d, must be PS_LOSS_DICE or PS_LOSS_DICE_WEIGHTED", who, (int)kind);
    PS_CHECK(c && logits && labels && sums, "%s: NULL argument", who);
    PS_CHECK(kind == PS_LOSS_DICE || class_weights, "%s: PS_LOSS_DICE_WEIGHTED needs class_weights", who);
    PS_CHECK(loss || dlogits, "%s: loss and dlogits are both NULL", who);
    PS_TRY(loss_shape_ok(who, R, C, kMaxClasses));
    PS_HIP(hipSetDevice(c->device));
    Stage st(c, "train_loss", 1);
    const int mode = dice_mode((int)C, logits, dlogits ? dlogits : logits);
    for (int64_t r0 = 0; r0 < (dlogits ? R : 1); r0 += kRowsPerLaunch) {  // (the loss comes from the first launch; without dlogits it is the only one)
        const int V = (int)std::min(kRowsPerLaunch, R - r0);
        const ValidWeight::Finish fin{kind == PS_LOSS_DICE_WEIGHTED ? class_weights : nullptr, (double)grad_scale, r0 == 0 ? loss : nullptr};
        const HardLabels lab{labels + r0};
        const float* lf = logits + r0 * C;
        float* out = dlogits ? dlogits + r0 * C : nullptr;
        const dim3 grid(dlogits ? (unsigned)ceil_div(V, 256) : 1u, 1);
        if (mode == 2) hipLaunchKernelGGL((dice_bwd_kernel<2, HardLabels, NoAct, ValidWeight>), grid, dim3(256), 0, c->stream, lf, lab, ValidWeight{}, sums, fin, 1, V, (int)C, out);
        else if (mode == 4) hipLaunchKernelGGL((dice_bwd_kernel<4, HardLabels, NoAct, ValidWeight>), grid, dim3(256), 0, c->stream, lf, lab, ValidWeight{}, sums, fin, 1, V, (int)C, out);
        else hipLaunchKernelGGL((dice_bwd_kernel<1, HardLabels, NoAct, ValidWeight>), grid, dim3(256), 0, c->stream, lf, lab, ValidWeight{}, sums, fin, 1, V, (int)C, out);
    }
    PS_HIP(hipGetLastError());
    return PS_OK;
}

extern "C" int ps_op_top1_counts(ps_context* c, const float* logits, const int32_t* labels, int64_t R, int64_t C, double* counts)
{
    using namespace ps;
    static const char* who = "ps_op_top1_counts";
    PS_CHECK(c && logits && labels && counts, "%s: NULL argument", who);
    PS_TRY(loss_shape_ok(who, R, C, 64));
    PS_HIP(hipSetDevice(c->device));
    const int slabs = ceil_div(R, kSlab);
    PS_TRY(c->red_ws.reserve(sizeof(double) * (size_t)slabs * 2));
    double* part = c->red_ws.as<double>();
    Stage st(c, "train_loss", 2);
    for (int64_t r0 = 0; r0 < R; r0 += kRowsPerLaunch) {
        const int V = (int)std::min(kRowsPerLaunch, R - r0);
        hipLaunchKernelGGL(top1_counts_kernel, dim3((unsigned)ceil_div(V, kSlab)), dim3(256), 0, c->stream, logits + r0 * C, labels + r0, V, (int)C,
                           part + (r0 / kSlab) * 2);
    }
    hipLaunchKernelGGL(reduce_partials_kernel<double>, dim3(1), dim3(256), 0, c->stream, part, slabs, 2, counts);
    PS_HIP(hipGetLastError());
    return PS_OK;
}
