// asan_map_main.cpp -- the host plan of ps_saliency_map under -fsanitize=address,undefined, with no GPU and no HIP call (`make asan-map`;
// tests/test_saliency_map_sanitizer.py runs it): the view axes, the window table and the scratch plan of saliency_map_plan.h over a spread
// of shapes.  Checks what ps_saliency_map relies on: the table is window_origins (eval.py:142-144) per view axis with axis 0 outermost,
// every window starts inside the volume unless a step exceeds the patch, and together they cover what the rule says; every scratch region
// is 256-byte aligned, inside the total the plan reports and disjoint from every other one.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "saliency_map_plan.h"

using namespace ps;

static int fail(const char* what, const char* a)
{
    std::fprintf(stderr, "asan_map_main: %s: %s\n", what, a);
    return 1;
}

// np.arange(0, max(1, n - patch + step), step), written as the loop it is
static std::vector<int64_t> window_origins(int64_t n, int64_t patch, int64_t step)
{
    std::vector<int64_t> o;
    for (int64_t at = 0; at < (n - patch + step > 1 ? n - patch + step : 1); at += step) o.push_back(at);
    return o;
}

static int check_table(int view, int64_t D, int64_t H, int64_t W, const int64_t* patch, const int64_t* step, int batch)
{
    MapPlan p;
    map_windows(view, D, H, W, patch, step, p);
    const int64_t ext[3] = {D, H, W};
    const int* ax = map_axis(view);
    int seen[3] = {0, 0, 0};
    std::vector<int64_t> org[3];
    for (int a = 0; a < 3; ++a) {
        if (ax[a] < 0 || ax[a] > 2 || seen[ax[a]]++) return fail("table", "the view's axes are no permutation");
        if (p.n[a] != ext[ax[a]]) return fail("table", "a view extent is not the volume's");
        org[a] = window_origins(p.n[a], patch[a], step[a]);
        if ((int64_t)org[a].size() != p.cnt[a]) return fail("table", "the origin count is not window_origins'");
    }
    if (p.windows != p.cnt[0] * p.cnt[1] * p.cnt[2]) return fail("table", "the window count");
    // the count of every view voxel, from the table and from the three origin lists
    std::vector<int> got((size_t)(p.n[0] * p.n[1] * p.n[2]), 0);
    int64_t t = 0, batches = 0;
    for (int64_t t0 = 0; t0 < p.windows; t0 += batch, ++batches) {
        const int64_t nb = batch < p.windows - t0 ? batch : p.windows - t0;
        if (nb < 1 || nb > batch) return fail("table", "a batch of the loop is empty or too large");
        for (int64_t b = 0; b < nb; ++b, ++t) {
            int64_t o[3];
            map_window_origin(p, t0 + b, o);
            const int64_t i0 = t / (p.cnt[1] * p.cnt[2]), i1 = t / p.cnt[2] % p.cnt[1], i2 = t % p.cnt[2];
            if (o[0] != org[0][(size_t)i0] || o[1] != org[1][(size_t)i1] || o[2] != org[2][(size_t)i2]) return fail("table", "a window's origin, or the window order");
            for (int a = 0; a < 3; ++a)
                if (o[a] < 0 || (o[a] >= p.n[a] && step[a] <= patch[a])) return fail("table", "a window starts outside the volume without a long step");
            for (int64_t i = o[0]; i < o[0] + patch[0] && i < p.n[0]; ++i)
                for (int64_t j = o[1]; j < o[1] + patch[1] && j < p.n[1]; ++j)
                    for (int64_t k = o[2]; k < o[2] + patch[2] && k < p.n[2]; ++k) got[(size_t)((i * p.n[1] + j) * p.n[2] + k)] += 1;
        }
    }
    if (t != p.windows || batches != (p.windows + batch - 1) / batch) return fail("table", "the batches do not tile the table");
    for (int64_t i = 0; i < p.n[0]; ++i)
        for (int64_t j = 0; j < p.n[1]; ++j)
            for (int64_t k = 0; k < p.n[2]; ++k) {
                int c[3] = {0, 0, 0};
                const int64_t at[3] = {i, j, k};
                for (int a = 0; a < 3; ++a)
                    for (int64_t o : org[a]) c[a] += o <= at[a] && at[a] < o + patch[a];
                if (got[(size_t)((i * p.n[1] + j) * p.n[2] + k)] != c[0] * c[1] * c[2]) return fail("table", "a voxel's cover");
                // a step of at most the patch leaves no hole
                if (step[0] <= patch[0] && step[1] <= patch[1] && step[2] <= patch[2] && c[0] * c[1] * c[2] < 1) return fail("table", "a hole without a long step");
            }
    return 0;
}

struct Region {
    const char* name;
    size_t at, bytes;
};

static int check_scratch(int64_t D, int64_t H, int64_t W, int64_t C, int64_t K, int n_views, const int64_t* patch, int batch, size_t fwd_bytes)
{
    MapPlan p;
    map_scratch(D, H, W, C, K, n_views, patch, batch, fwd_bytes, p);
    const size_t vox = (size_t)D * H * W, win = (size_t)patch[0] * patch[1] * patch[2];
    if (p.map_bytes != vox * K * 4 || p.count_bytes != vox * 4 || p.x_bytes != batch * win * C * 4 || p.probs_bytes != batch * win * K * 4)
        return fail("scratch", "a region's size");
    if ((n_views > 1) != (p.run_bytes != 0)) return fail("scratch", "the running fusion exists exactly with more than one view");
    const Region r[] = {{"sum", p.sum, p.map_bytes}, {"run", p.run, p.run_bytes}, {"count", p.count, p.count_bytes},
                        {"x", p.x, p.x_bytes},       {"probs", p.probs, p.probs_bytes}, {"fwd", p.fwd, p.fwd_bytes}};
    if (p.total % 256) return fail("scratch", "the total is no multiple of 256");
    std::vector<unsigned char> owner(p.total / 256, 0);
    for (const Region& g : r) {
        if (g.at % 256) return fail("scratch", g.name);
        if (g.at + g.bytes > p.total) return fail("scratch", g.name);
        for (size_t b = g.at / 256; b < (g.at + g.bytes + 255) / 256; ++b) {
            if (owner[b]) return fail("scratch overlap", g.name);
            owner[b] = 1;
        }
    }
    for (size_t b = 0; b < owner.size(); ++b)
        if (!owner[b]) return fail("scratch", "a block belongs to no region");
    // beside out: at most two maps and one count, then the windows and the forward's scratch
    if (p.total > 2 * map_pad256(p.map_bytes) + map_pad256(p.count_bytes) + map_pad256(p.x_bytes) + map_pad256(p.probs_bytes) + map_pad256(fwd_bytes))
        return fail("scratch", "more than the header promises");
    return 0;
}

int main()
{
    struct Case {
        int64_t D, H, W, patch[3], step[3];
    };
    const Case cases[] = {
        {23, 40, 50, {16, 32, 32}, {12, 24, 24}},   // the tests' base case: 8 / 8 / 6 windows
        {10, 20, 30, {16, 32, 32}, {12, 24, 24}},   // smaller than the patch
        {23, 40, 1, {16, 32, 32}, {12, 24, 24}},    // an extent of 1
        {1, 1, 1, {16, 16, 16}, {1, 1, 1}},
        {40, 37, 45, {16, 16, 16}, {20, 17, 33}},   // steps larger than the patch: holes
        {33, 17, 48, {16, 16, 32}, {5, 16, 7}},
        {64, 160, 160, {64, 160, 160}, {48, 118, 118}},
        {70, 61, 59, {32, 48, 16}, {48, 118, 118}},
    };
    for (const Case& c : cases)
        for (int view = 0; view < 3; ++view)
            for (int batch : {1, 2, 3, 5, 8}) {
                if (check_table(view, c.D, c.H, c.W, c.patch, c.step, batch)) return 1;
                for (int n_views = 1; n_views <= 3; ++n_views)
                    for (size_t fwd : {(size_t)0, (size_t)1, (size_t)123457})
                        for (int K : {2, 3, 16})
                            if (check_scratch(c.D, c.H, c.W, view + 1, K, n_views, c.patch, batch, fwd)) return 1;
            }
    std::printf("asan_map_main ok\n");
    return 0;
}
