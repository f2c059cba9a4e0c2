// randla_net.h -- the network object behind the opaque ps_randla handle (randla.hip): the layer table of the weight blob and the
// packed weight images of every layer.  Shared with the test-only library (debug_hooks.hip), whose ps_debug_att_stage runs one
// attention stage on a live network's own images.
#pragma once

#include <memory>
#include <vector>

#include "attpool.h"
#include "common.h"
#include "rowgemm.h"

namespace ps {

struct LayerSpec {
    int cin, cout, leaky;
    size_t w_off, b_off;  // offsets into the host blob (floats)
};

struct EncLevel {
    PackedLinear mlp1, top1, lfa1, bot1, full1, att1mlp, lfa2, top2, bot2, full2, att2mlp, mlp2sc;
    // images at PS_PREC_BF16 only: Wfc1[:h, :] / Wfc2[:h, :] UNROUNDED, for a level whose rows the 32x32 attention kernels do not fit at run
    // time -- its stage runs as at the default precision, and so does its score pre-product G (top1 / top2 are the rounded ones there)
    PackedLinear top1x, top2x;
    Att32Weights p32;  // d >= 64: weight images of the 32x32x2 attentive-pooling kernels
    bool has_p32 = false;
    const float *lane1 = nullptr, *lane2 = nullptr;  // d = 16: plain fp32 images of the two attention stages (attpool_lane.hip: pack_lane_image)
    int d_in, d;
};

// every packed weight image of a network at one precision (ps_randla_set_weights packs the default ones, the first forward at PS_PREC_BF16
// the others), with the chain images built from them
struct NetImages {
    DevBuf wbuf;
    ChainCache chains;  // re-ordered weight images of the register-resident layer chains (regchain.hip)
    PackedLinear fc0, decoder0, fc1, fc2, fc;
    std::vector<EncLevel> enc;
    std::vector<PackedLinear> dec;
    void release()
    {
        wbuf.release();
        chains.clear();
    }
};

}  // namespace ps

struct ps_randla;
namespace ps {
// packs net->bf16, the images of PS_PREC_BF16, from the kept blob unless they exist (randla.hip); the weights must be set
int randla_bf16_images(ps_randla* net);
}  // namespace ps

struct ps_randla : ps::NetImages {  // (the base: the images of the default precision)
    ps_context* ctx = nullptr;
    ps_randla_config cfg;
    std::vector<ps::LayerSpec> specs;  // blob order
    int64_t blob_floats = 0;
    bool have_weights = false;
    // include/pointseg_forward_precision.h: PS_PREC_BF16X3 (the default) or PS_PREC_BF16; the one-plane images of the latter are packed from
    // the kept blob by the first forward that needs them and dropped by ps_randla_set_weights
    int precision = 1;
    std::vector<float> blob;
    std::unique_ptr<ps::NetImages> bf16;
    // taps of the last forward (device pointers into ctx->net_arena) and their sizes
    struct Tap { int which; const float* p; int64_t count; };
    std::vector<Tap> taps;
    bool keep_taps = false;  // ps_randla_keep_taps: also store the rows only ps_randla_tap reads (last decoder step)
};
