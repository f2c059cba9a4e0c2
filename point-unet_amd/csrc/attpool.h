// attpool.h -- fused LocSE + gather + attentive pooling (see attpool.hip).
#pragma once

#include "common.h"
#include "rowgemm.h"

namespace ps {

// Weight images of one encoder level for the 32x32x2 kernels (attpool32.hip: pack_p32 / pack_p32_locse), device pointers.
struct Att32Weights {
    const float* w1 = nullptr;   // LocSE mlp1 (10 -> h)
    const float* w2 = nullptr;   // LFA mlp2 (h -> h)
    const float* wb1 = nullptr;  // att_pooling_1 Wfc[h:, :] (h -> d)
    const float* wb2 = nullptr;  // att_pooling_2 Wfc[h:, :]
    // the same four matrices as three-plane bfloat16 images (attpool32b.hip: pack_b3 / pack_b3_locse); null when not packed
    const float* w1b = nullptr;
    const float* w2b = nullptr;
    const float* wb1b = nullptr;
    const float* wb2b = nullptr;
    // w2, wb1, wb2 rounded once to bfloat16 as ONE-plane images (pack_b3 with planes = 1) for the P = 1 kernels of attpool32b.hip: only the
    // images of a network at PS_PREC_BF16 carry them (LocSE has none: it stays on w1b)
    const float* w2b1 = nullptr;
    const float* wb1b1 = nullptr;
    const float* wb2b1 = nullptr;
};
void pack_b3(const float* W, int cin, int cout, uint16_t* out, int planes = 3);   // [cin, cout], cin % 32 == 0, cout % 32 == 0 -> cin*cout*planes uint16
void pack_b3_locse(const float* W1, int cout, uint16_t* out);     // [10, cout] -> (cout/32)*3*64*8 uint16
void pack_p32(const float* W, int cin, int cout, float* out);   // [cin, cout] row-major, cin % 8 == 0, cout % 32 == 0 -> cin*cout floats
void pack_p32_locse(const float* W1, int cout, float* out);     // [10, cout] -> (cout/32)*5*64 floats

struct AttStage {
    const float* xyz = nullptr;      // [n_total, 3]
    const int32_t* idx = nullptr;    // [n_total, k] cloud-local neighbour indices
    const int32_t* order = nullptr;  // optional [n_total]: cloud-local row of the t-th point in a spatially coherent order (ps_pyramid.order)
    const float* fg = nullptr;       // [n_total, d/2 + d]: features f | G = f . Wfc[:d/2, :]
    const PackedLinear* lfa1 = nullptr;  // 10 -> d/2 (bias + folded BN, LeakyReLU)
    const PackedLinear* lfa2 = nullptr;  // d/2 -> d/2, stage 2 only (nullptr = stage 1)
    const PackedLinear* wbot = nullptr;  // Wfc[d/2:, :]  (d/2 -> d, no bias): pre-product formulation, fg = [f | G]
    const PackedLinear* wfull = nullptr; // Wfc (d -> d): direct formulation, fg = f only (row stride ldf)
    int ldf = 0;
    float* agg = nullptr;            // [n_total, d]
    int64_t n_total = 0, n_cloud = 0;
    int d = 0, k = 16;
    const Att32Weights* p32 = nullptr;  // when set (d >= 64, pre-product formulation): the 32x32x2 kernels (attpool32.hip)
    const float* lane = nullptr;        // when set (d = 16, direct formulation): the stage's plain fp32 image (attpool_lane.hip: pack_lane_image)
    // the network runs at PS_PREC_BF16: a stage the split-bf16 32x32 kernels fit (att_pool32b_fits) takes their one-plane form, whatever the
    // context's att_bf16x3 says; any other stage runs as it does at the default precision
    int one_plane = 0;
};

// Plain fp32 image of one d = 16 attention stage for att_lane_kernel (attpool_lane.hip), offsets in floats: b1 [8] | W1 [10, 8] | b2 [8] |
// W2 [8, 8] | Wfc [16, 16] times log2(e), all row-major [cin, cout]: 13 chunks of 32 floats, the unit the kernel fetches.  b2 / W2 are zero
// in a stage-1 image.
constexpr int kLaneB1 = 0, kLaneW1 = 8, kLaneB2 = 88, kLaneW2 = 96, kLaneWfc = 160, kLaneImageFloats = 416;
void pack_lane_image(const float* W1, const float* b1, const float* W2, const float* b2, const float* wfc_scaled, float* out);

bool att_pool32_fits(const AttStage& s);
int att_pool32_stage(ps_context* c, const AttStage& s);
bool att_pool32b_fits(const AttStage& s);
int att_pool32b_stage(ps_context* c, const AttStage& s);

// the vector-ALU kernel of attpool_lane.hip (one lane per neighbour row): d = 16, K = 16, direct formulation, the context's att_lane switch on
bool att_lane_fits(const ps_context* c, const AttStage& s);
int att_lane_stage(ps_context* c, const AttStage& s);  // (PS_EINVAL outside d = 16 / K = 16 / direct, whatever the knob says)
int att_lane_pass_points();  // points one pass of its grid covers (beyond that a wave loops)

// the 32x32 forms when they fit (the split-bf16 one first, when the context asks for it), the lane form at d = 16 / K = 16, otherwise
// att_pool16_stage; att_pool_form names the choice as ps_debug_att_stage numbers its forms (1 bf16x3, 2 32x32, 3 16x16x4, 4 lane, 5 one-plane 32x32)
int att_pool_stage(ps_context* c, const AttStage& s);
int att_pool_form(const ps_context* c, const AttStage& s);
// the 16x16x4 kernels of attpool.hip: the direct formulation when wfull is set (d <= 32), otherwise the pre-product kernel att_kernel --
// what a level too large for the 32x32 forms (2^24 rows, 4 GiB of fg) runs
int att_pool16_stage(ps_context* c, const AttStage& s);

}  // namespace ps
