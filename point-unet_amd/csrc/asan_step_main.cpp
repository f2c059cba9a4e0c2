// asan_step_main.cpp -- the host side of the saliency training step under -fsanitize=address,undefined, with no GPU and no HIP call
// (`make asan-step`; tests/test_saliency_step_sanitizer.py runs it): the layer table, the optimiser's decay table and the scratch plan
// of saliency_step_plan.h over a range of shapes.  Checks what the walker relies on: every region 256-byte aligned, inside the total,
// and disjoint from every other one except the two stated aliases; the decay table equal to a walk over the layers.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "saliency_step_plan.h"

using namespace ps;

struct Region {
    const char* name;
    size_t at, bytes;
};

static int fail(const char* what, const char* a, const char* b = "")
{
    std::fprintf(stderr, "asan_step_main: %s: %s %s\n", what, a, b);
    return 1;
}

static int check_plan(int B, int D, int H, int W, int C_in, int K, size_t ops_bytes)
{
    Net net;
    build_net(net, C_in, K);
    StepPlan p;
    step_plan(net, B, D, H, W, K, ops_bytes, p);
    std::vector<Region> r;
    auto fl = [&](int l, int C) { return (size_t)B * p.Vl[l] * C * sizeof(float); };
    for (int i = 0; i < net.n; ++i) {
        if (p.level[i] < 0) continue;
        r.push_back({"X", p.X[i], fl(p.level[i], net.L[i].cout)});
        if (net.L[i].g >= 0) r.push_back({"Y", p.Y[i], fl(p.level[i], net.L[i].cout)});
        else if (p.Y[i] != p.X[i]) return fail("plan", "a layer without norm has a Y of its own");
    }
    for (int l = 0; l < 5; ++l) {
        r.push_back({"dn", p.dn[l], fl(l, 16 << l)});
        r.push_back({"gdn", p.gdn[l], fl(l, 16 << l)});
        if (l) r.push_back({"tA", p.tA[l], fl(l, 16 << l)}), r.push_back({"tB", p.tB[l], fl(l, 16 << l)});
    }
    if (p.tA[0] != p.gA || p.tB[0] != p.gC) return fail("plan", "level 0's temporaries are not gA and gC");
    r.push_back({"cfecat1", p.cfecat[1], fl(3, 128)}), r.push_back({"cfecat2", p.cfecat[2], fl(4, 128)});
    r.push_back({"cat345", p.cat345, fl(2, kCA)}), r.push_back({"ca_y", p.ca_y, fl(2, kCA)});
    r.push_back({"mean", p.mean, (size_t)B * kCA * 4}), r.push_back({"hidden", p.hidden, (size_t)B * kCAh * 4}), r.push_back({"scale", p.scale, (size_t)B * kCA * 4});
    r.push_back({"sa_map", p.sa_map, fl(0, 1)}), r.push_back({"gated", p.gated, fl(0, 64)}), r.push_back({"logits", p.logits, fl(0, K)});
    r.push_back({"sums", p.sums, (size_t)B * K * 3 * 8});
    r.push_back({"gK", p.gK, fl(0, K)});
    r.push_back({"gA", p.gA, fl(0, 64)}), r.push_back({"gB", p.gB, fl(0, 64)}), r.push_back({"gC", p.gC, fl(0, 64)}), r.push_back({"gD", p.gD, fl(0, 64)});
    r.push_back({"gS", p.gS, fl(0, 32)}), r.push_back({"g1", p.g1, fl(0, 1)}), r.push_back({"g1b", p.g1b, fl(0, 1)}), r.push_back({"g1c2", p.g1c2, fl(1, 64)});
    r.push_back({"g2c", p.g2c, fl(2, 64)}), r.push_back({"g2cat", p.g2cat, fl(2, kCA)}), r.push_back({"g2p", p.g2p, fl(2, 128)}), r.push_back({"g2b", p.g2b, fl(2, 32)});
    r.push_back({"g3cfe", p.g3cfe, fl(3, 128)}), r.push_back({"g3b", p.g3b, fl(3, 32)}), r.push_back({"g4cfe", p.g4cfe, fl(4, 128)}), r.push_back({"g4b", p.g4b, fl(4, 32)});
    r.push_back({"ops", p.ops, ops_bytes});
    // what the walker writes through: a byte per 256-byte block of the scratch, marked by its owner
    std::vector<unsigned char> owner(p.total / 256, 0);
    if (p.total % 256) return fail("plan", "the total is no multiple of 256");
    for (const Region& g : r) {
        if (g.at % 256) return fail("plan", g.name, "is not 256-byte aligned");
        if (g.at + g.bytes > p.total) return fail("plan", g.name, "ends behind the total");
        for (size_t b = g.at / 256; b < (g.at + g.bytes + 255) / 256; ++b) {
            if (owner[b]) return fail("plan", g.name, "overlaps another region");
            owner[b] = 1;
        }
    }
    for (size_t b = 0; b < owner.size(); ++b)
        if (!owner[b]) return fail("plan", "a block of the scratch belongs to no region");
    return 0;
}

static int check_decay(int C_in, int K)
{
    Net net;
    build_net(net, C_in, K);
    if (net.n > 48 || net.count >= (1ll << 31)) return fail("decay", "the network outgrew the table");
    DecayTable t;
    decay_table(net, t);
    std::vector<unsigned char> want((size_t)net.count, 0);
    for (int i = 0; i < net.n; ++i) {
        const Layer& l = net.L[i];
        const int64_t n = (int64_t)l.kd * l.kh * l.kw * l.cin * l.cout;
        for (int64_t e = l.w; e < l.w + n; ++e) want[(size_t)e] = 1;
        int64_t end = l.w + n + (l.b >= 0 ? l.cout : 0) + (l.g >= 0 ? 2 * l.cout : 0);
        if (end != (i + 1 < net.n ? net.L[i + 1].w : net.count)) return fail("decay", "the layers do not tile the buffer");
    }
    for (int j = 1; j < 96; ++j)
        if (t.bound[j] < t.bound[j - 1]) return fail("decay", "the bounds do not ascend");
    // the kernel's rule at every bound, its neighbours, and a stride through the rest
    auto decays = [&](int64_t e) {
        int n = 0;
        for (int j = 0; j < 96; ++j) n += t.bound[j] <= e ? 1 : 0;
        return n & 1;
    };
    for (int j = 0; j < 2 * net.n; ++j)
        for (int64_t e = (int64_t)t.bound[j] - 2; e <= (int64_t)t.bound[j] + 2; ++e)
            if (e >= 0 && e < net.count && decays(e) != want[(size_t)e]) return fail("decay", "the parity rule disagrees at a bound");
    for (int64_t e = 0; e < net.count; e += 997)
        if (decays(e) != want[(size_t)e]) return fail("decay", "the parity rule disagrees");
    return 0;
}

int main()
{
    const int shapes[][4] = {{1, 16, 16, 16}, {2, 32, 16, 16}, {1, 16, 48, 32}, {2, 64, 160, 160}, {3, 16, 16, 80}};
    for (const auto& s : shapes)
        for (int K : {2, 3, 4, 16})
            for (size_t ops : {(size_t)0, (size_t)1, (size_t)123457}) {
                if (s[2] == 160 && (K != 2 || ops != 1)) continue;  // (the reference's batch once: its plan is 16 GB of blocks to mark)
                if (check_plan(s[0], s[1], s[2], s[3], 1, K, ops)) return 1;
            }
    for (int C_in : {1, 2, 4, 16})
        for (int K : {2, 3, 4, 16})
            if (check_decay(C_in, K)) return 1;
    std::printf("asan_step_main ok\n");
    return 0;
}
