// randla_net.h -- the network object behind the opaque ps_randla handle (randla.hip): the layer table of the weight blob and the
// packed weight images of every layer.  Shared with the test-only library (debug_hooks.hip), whose ps_debug_att_stage runs one
// attention stage on a live network's own images.
#pragma once

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
    Att32Weights p32;  // d >= 64: weight images of the 32x32x2 attentive-pooling kernels
    bool has_p32 = false;
    const float *lane1 = nullptr, *lane2 = nullptr;  // d = 16: plain fp32 images of the two attention stages (attpool_lane.hip: pack_lane_image)
    int d_in, d;
};

}  // namespace ps

struct ps_randla {
    ps_context* ctx = nullptr;
    ps_randla_config cfg;
    std::vector<ps::LayerSpec> specs;  // blob order
    int64_t blob_floats = 0;
    bool have_weights = false;
    ps::DevBuf wbuf;
    ps::ChainCache chains;  // re-ordered weight images of the register-resident layer chains (regchain.hip)
    ps::PackedLinear fc0, decoder0, fc1, fc2, fc;
    std::vector<ps::EncLevel> enc;
    std::vector<ps::PackedLinear> dec;
    // taps of the last forward (device pointers into ctx->net_arena) and their sizes
    struct Tap { int which; const float* p; int64_t count; };
    std::vector<Tap> taps;
    bool keep_taps = false;  // ps_randla_keep_taps: also store the rows only ps_randla_tap reads (last decoder step)
};
