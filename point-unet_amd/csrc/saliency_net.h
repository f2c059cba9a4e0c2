// saliency_net.h -- the layer table of unet3d_attention in the order of the flat weight buffer (include/pointseg_saliency.h), shared by
// saliency.hip (the inference forward) and saliency_step.hip (the training step), and the table of the segments of that buffer the
// optimiser decays (include/pointseg_saliency_step.h).  Host code only, no HIP: a plain C++ compiler takes it (asan_step_main.cpp).
#pragma once
#include <cstdint>

namespace ps {

constexpr int kCA = 384, kCAh = 96, kC345 = 64;

struct Layer {
    int kd, kh, kw, cin, cout;
    int64_t w, b, g, be;  // offsets into the weight buffer; -1: the layer has none
};

struct Net {
    Layer L[48];
    int n = 0;
    int64_t count = 0;
    int init, down[5][2], s2[4], c1, c2, cfe[3][4], up5, up4, d1, d2, c345, up345, sa[3][2], upc2, c12, fin;
};

inline int add_layer(Net& n, int kd, int kh, int kw, int cin, int cout, bool bias, bool norm)
{
    Layer& l = n.L[n.n];
    l = {kd, kh, kw, cin, cout, n.count, -1, -1, -1};
    n.count += (int64_t)kd * kh * kw * cin * cout;
    if (bias) l.b = n.count, n.count += cout;
    if (norm) {
        l.g = n.count, n.count += cout;
        l.be = n.count, n.count += cout;
    }
    return n.n++;
}

// the order of include/pointseg_saliency.h
inline void build_net(Net& n, int cin, int classes)
{
    n.init = add_layer(n, 3, 3, 3, cin, 16, true, true);
    for (int d = 0; d < 5; ++d) {
        const int w = 16 << d;
        n.down[d][0] = add_layer(n, 3, 3, 3, w, w, true, true);
        n.down[d][1] = add_layer(n, 3, 3, 3, w, w, true, true);
        if (d < 4) n.s2[d] = add_layer(n, 3, 3, 3, w, 2 * w, true, true);
    }
    n.c1 = add_layer(n, 3, 3, 3, 16, 64, true, true);
    n.c2 = add_layer(n, 3, 3, 3, 32, 64, true, true);
    for (int p = 0; p < 3; ++p) {
        n.cfe[p][0] = add_layer(n, 1, 1, 1, 64 << p, 32, false, true);
        for (int r = 1; r < 4; ++r) n.cfe[p][r] = add_layer(n, 3, 3, 3, 64 << p, 32, false, true);
    }
    n.up5 = add_layer(n, 3, 3, 3, 128, 128, true, true);
    n.up4 = add_layer(n, 3, 3, 3, 128, 128, true, true);
    n.d1 = add_layer(n, 1, 1, 1, kCA, kCAh, true, false);
    n.d2 = add_layer(n, 1, 1, 1, kCAh, kCA, true, false);
    n.c345 = add_layer(n, 1, 1, 1, kCA, kC345, true, true);
    n.up345 = add_layer(n, 3, 3, 3, 64, 64, true, true);
    const int k1[3][3] = {{1, 9, 9}, {9, 1, 9}, {9, 9, 1}}, k2[3][3] = {{9, 1, 1}, {1, 9, 1}, {1, 1, 9}};
    for (int i = 0; i < 3; ++i) {
        n.sa[i][0] = add_layer(n, k1[i][0], k1[i][1], k1[i][2], 64, 32, true, true);
        n.sa[i][1] = add_layer(n, k2[i][0], k2[i][1], k2[i][2], 32, 1, true, true);
    }
    n.upc2 = add_layer(n, 3, 3, 3, 64, 64, true, true);
    n.c12 = add_layer(n, 3, 3, 3, 128, 64, true, true);
    n.fin = add_layer(n, 3, 3, 3, 128, classes, true, false);
}

inline bool net_args_ok(int64_t C_in, int64_t classes) { return C_in >= 1 && C_in <= 16 && classes >= 2 && classes <= 16; }

// The `/kernel` tensors of the weight buffer, ascending: element e decays exactly when bound[2 s] <= e < bound[2 s + 1] for some layer s,
// that is, when an odd number of bounds are <= e.  The unused entries are INT_MAX; the buffer has fewer than 2^31 elements (about 10^7).
// 48 layers at the most, so the table travels as a kernel argument.
struct DecayTable {
    int bound[96];
};

inline void decay_table(const Net& net, DecayTable& t)
{
    for (int i = 0; i < net.n; ++i) {
        const Layer& l = net.L[i];
        t.bound[2 * i] = (int)l.w;
        t.bound[2 * i + 1] = (int)(l.w + (int64_t)l.kd * l.kh * l.kw * l.cin * l.cout);
    }
    for (int i = 2 * net.n; i < 96; ++i) t.bound[i] = 0x7fffffff;
}

}  // namespace ps
