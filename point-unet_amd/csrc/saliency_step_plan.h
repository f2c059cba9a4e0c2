// saliency_step_plan.h -- where everything of one training step lies in the caller's scratch (include/pointseg_saliency_step.h,
// DESIGN.md 4.13): a function of the shapes alone.  Host code only, no HIP: a plain C++ compiler takes it (asan_step_main.cpp).
//
// Kept for the backward: per layer the convolution's output X and the norm's output Y; the five down_list tensors; the concats; the
// channel attention's mean / hidden / scale and its scaled tensor; the spatial attention and the gated C12; the logits and the Dice sums.
// Gradient workspaces, per level l (extent >> l, width w = 16 << l): gdn[l] the gradient of down_list[l] (later of the block's input),
// tA[l] and tB[l] two temporaries of the block; and the buffers of the decoder named below.  At level 0 tA and tB are gA and gC, which the
// decoder has left by the time the encoder's backward starts.  Everything is a multiple of 256 bytes from the scratch's start.
#pragma once
#include <cstddef>
#include <cstdint>

#include "saliency_net.h"

namespace ps {

struct StepPlan {
    int B, K, Dl[5], Hl[5], Wl[5], Vl[5];
    int level[48];         // the level of each layer's OUTPUT (-1: the two dense layers, which have no tensor)
    size_t X[48], Y[48];   // byte offsets; Y == X where the layer has no norm
    size_t dn[5], cfecat[3], cat345, mean, hidden, scale, ca_y, sa_map, gated, logits, sums;
    size_t gK, gA, gB, gC, gD, gS, g1, g1b, g1c2, g2c, g2cat, g2p, g2b, g3cfe, g3b, g4cfe, g4b, gdn[5], tA[5], tB[5];
    size_t ops, ops_bytes, total;
};

inline size_t plan_pad256(size_t n) { return (n + 255) & ~(size_t)255; }

inline void step_plan(const Net& net, int B, int D, int H, int W, int K, size_t ops_bytes, StepPlan& p)
{
    p.B = B, p.K = K;
    for (int l = 0; l < 5; ++l) p.Dl[l] = D >> l, p.Hl[l] = H >> l, p.Wl[l] = W >> l, p.Vl[l] = p.Dl[l] * p.Hl[l] * p.Wl[l];
    for (int i = 0; i < 48; ++i) p.level[i] = -1, p.X[i] = p.Y[i] = 0;
    p.level[net.init] = 0;
    for (int d = 0; d < 5; ++d) {
        p.level[net.down[d][0]] = p.level[net.down[d][1]] = d;
        if (d < 4) p.level[net.s2[d]] = d + 1;
    }
    p.level[net.c1] = 0, p.level[net.c2] = 1;
    for (int q = 0; q < 3; ++q)
        for (int r = 0; r < 4; ++r) p.level[net.cfe[q][r]] = 2 + q;
    p.level[net.up5] = p.level[net.up4] = p.level[net.c345] = 2;
    p.level[net.up345] = p.level[net.upc2] = p.level[net.c12] = p.level[net.fin] = 0;
    for (int i = 0; i < 3; ++i) p.level[net.sa[i][0]] = p.level[net.sa[i][1]] = 0;

    size_t off = 0;
    auto bytes = [&](size_t n) {
        const size_t at = off;
        off += plan_pad256(n);
        return at;
    };
    auto floats = [&](int l, int C) { return bytes((size_t)B * p.Vl[l] * C * sizeof(float)); };
    for (int i = 0; i < net.n; ++i) {
        if (p.level[i] < 0) continue;
        p.X[i] = floats(p.level[i], net.L[i].cout);
        p.Y[i] = net.L[i].g >= 0 ? floats(p.level[i], net.L[i].cout) : p.X[i];
    }
    for (int l = 0; l < 5; ++l) p.dn[l] = floats(l, 16 << l);
    p.cfecat[0] = 0;  // (C3_cfe's branches go straight into cat345)
    p.cfecat[1] = floats(3, 128), p.cfecat[2] = floats(4, 128);
    p.cat345 = floats(2, kCA), p.ca_y = floats(2, kCA);
    p.mean = bytes((size_t)B * kCA * sizeof(float)), p.hidden = bytes((size_t)B * kCAh * sizeof(float)), p.scale = bytes((size_t)B * kCA * sizeof(float));
    p.sa_map = floats(0, 1), p.gated = floats(0, 64);
    p.logits = floats(0, K);
    p.sums = bytes((size_t)B * K * 3 * sizeof(double));
    p.gK = floats(0, K);
    p.gA = floats(0, 64), p.gB = floats(0, 64), p.gC = floats(0, 64), p.gD = floats(0, 64);
    p.gS = floats(0, 32), p.g1 = floats(0, 1), p.g1b = floats(0, 1);
    p.g1c2 = floats(1, 64);
    p.g2c = floats(2, 64), p.g2cat = floats(2, kCA), p.g2p = floats(2, 128), p.g2b = floats(2, 32);
    p.g3cfe = floats(3, 128), p.g3b = floats(3, 32), p.g4cfe = floats(4, 128), p.g4b = floats(4, 32);
    for (int l = 0; l < 5; ++l) {
        p.gdn[l] = floats(l, 16 << l);
        p.tA[l] = l ? floats(l, 16 << l) : p.gA;
        p.tB[l] = l ? floats(l, 16 << l) : p.gC;
    }
    p.ops = bytes(ops_bytes);
    p.ops_bytes = ops_bytes;
    p.total = off;
}

}  // namespace ps
