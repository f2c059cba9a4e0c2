// debug_hooks.hip -- the TEST-ONLY library libpointseg_debug.so (declarations: debug_hooks.h): doors used by the test-suite to
// exercise the product's OWN host logic without a GPU -- the kd-tree construction rules (kdtree_host.hip) and the per-query
// search routine that the HIP kernel instantiates (kdtree.h, __host__ __device__) --, to read a device-built tree back, and to launch
// kernel forms of the forward on their own (one dense layer, a layer chain, an attention stage) that the network picks by shape.
// Built next to the product library and linked against it; nothing in the product library or the Python package refers to it
// (tests/conftest.py binds it) -- it is not a CPU fallback.  The two pure-host doors (ps_debug_knn_host, ps_debug_kdtree_host) live
// in debug_host.hip, which is also built on its own under the host sanitizers (`make asan-host`).
#include "common.h"

#include <cstring>
#include <vector>
#include "kdtree_build.h"
#include "kdtree_host.h"
#include "rowgemm.h"
#include "attpool.h"
#include "b3_ops.h"
#include "debug_hooks.h"
#include "randla_net.h"
#include "reduce_partials.h"
#include "sortscan.h"

using namespace ps;

extern "C" int ps_debug_volume_sample_args_size(void) { return (int)sizeof(ps_volume_sample_args); }

extern "C" int ps_debug_pack_weights(const float* W, int cin, int cout, int ntb, float* out)
{
    PS_CHECK(W && out && (ntb == 1 || ntb == 2 || ntb == 4), "ps_debug_pack_weights: bad argument");
    pack_weights(W, cin, cout, ntb, out);
    return PS_OK;
}

extern "C" int ps_debug_pack_b3(const float* W, int cin, int cout, uint16_t* out)
{
    PS_CHECK(W && out && cin > 0 && cin % 32 == 0 && cout > 0 && cout % 32 == 0, "ps_debug_pack_b3: bad argument");
    pack_b3(W, cin, cout, out);
    return PS_OK;
}

// the same image from the DEVICE split (b3_split8 through pack_batch_b3's kind 5, the accumulator K order that pack_b3 writes too)
extern "C" int ps_debug_pack_b3_device(ps_context* c, const float* W, int cin, int cout, void* out)
{
    PS_CHECK(c && W && out && cin > 0 && cin % 32 == 0 && cout > 0 && cout % 32 == 0, "ps_debug_pack_b3_device: bad argument");
    PS_HIP(hipSetDevice(c->device));
    PackJob j{};
    j.w = W; j.sk = cout; j.sn = 1; j.kind = 5; j.cin = cin; j.cout = cout; j.out = out;
    j.total = (int64_t)(cin / 16) * (cout / 32) * 64;
    PackJob* table = nullptr;
    PS_HIP(hipMalloc(reinterpret_cast<void**>(&table), sizeof(PackJob)));
    int rc = hipMemcpy(table, &j, sizeof(PackJob), hipMemcpyHostToDevice) == hipSuccess ? pack_batch_b3(c, table, 1) : PS_EINVAL;
    (void)hipStreamSynchronize(c->stream);
    (void)hipFree(table);
    return rc;
}

// one dense layer through gemm32b.hip / gemm32.hip with freshly packed weight images (the product packs them once per network)
extern "C" int ps_debug_gemm32(ps_context* c, int split_bf16, const float* x1, int ld1, int c1, const int32_t* g1, const float* x2, int ld2, int c2,
                               const int32_t* g2, int gm, int gn, const float* W, const float* bias, int64_t R, int cout, int leaky, float* y, int ldy)
{
    PS_CHECK(c && x1 && W && bias && y && R >= 0 && c1 > 0 && c2 >= 0 && cout > 0, "ps_debug_gemm32: bad argument");
    PS_HIP(hipSetDevice(c->device));
    const int cin = c1 + c2;
    // (gemm32_fits: 8-wide K chunks for the fp32 kernel, 16-wide for the split form)
    PS_CHECK(split_bf16 >= 0 && split_bf16 <= 2, "ps_debug_gemm32: split_bf16 is 0, 1 or 2");
    PS_CHECK(cin % (split_bf16 ? 16 : 8) == 0 && cout % 32 == 0, "ps_debug_gemm32: cin %% %d and cout %% 32 must be 0", split_bf16 ? 16 : 8);
    const bool one_plane = split_bf16 == 2;  // (the image of a rounded layer: pack_p32b rounds the weights itself)
    std::vector<float> img((size_t)cin * cout * (one_plane ? 1 : (split_bf16 ? 3 : 2)) / 2);
    if (split_bf16) pack_p32b(W, cin, cout, reinterpret_cast<uint16_t*>(img.data()), one_plane ? 1 : 3);
    else pack_p32(W, cin, cout, img.data());
    float *d_img = nullptr, *d_bias = nullptr;
    PS_HIP(hipMalloc(reinterpret_cast<void**>(&d_img), img.size() * sizeof(float)));
    PS_HIP(hipMalloc(reinterpret_cast<void**>(&d_bias), sizeof(float) * (size_t)cout));
    PS_HIP(hipMemcpyAsync(d_img, img.data(), img.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    PS_HIP(hipMemcpyAsync(d_bias, bias, sizeof(float) * (size_t)cout, hipMemcpyHostToDevice, c->stream));
    PackedLinear L;
    L.cin = cin; L.cout = cout; L.leaky = leaky; L.bias = d_bias;
    if (one_plane) { L.w32b1 = d_img; L.round = 1; }
    else if (split_bf16) L.w32b = d_img;
    else L.w32 = d_img;
    RowSrc s1, s2;
    s1.x = x1; s1.ld = ld1; s1.c = c1; s1.gather = g1; s1.gm = g1 ? gm : 0; s1.gn = g1 ? gn : 0;
    s2.x = x2; s2.ld = ld2; s2.c = c2; s2.gather = g2; s2.gm = g2 ? gm : 0; s2.gn = g2 ? gn : 0;
    int rc = PS_EINVAL;
    if (split_bf16 ? gemm32b_fits(L, s1, s2, R, ldy) : gemm32_fits(L, s1, s2, R, ldy))
        rc = split_bf16 ? gemm32b(c, L, s1, s2, R, y, ldy) : gemm32(c, L, s1, s2, R, y, ldy);
    else
        set_error("ps_debug_gemm32: the shape does not fit the kernel");
    (void)hipStreamSynchronize(c->stream);
    (void)hipFree(d_img);
    (void)hipFree(d_bias);
    return rc;
}

extern "C" int ps_debug_gemm32_plan(ps_context* c, int split_bf16, int64_t R, int cin, int cout, int* out4)
{
    PS_CHECK(c && out4 && R >= 1 && cin > 0 && cout > 0 && split_bf16 >= 0 && split_bf16 <= 2 && cin % (split_bf16 ? 16 : 8) == 0 && cout % 32 == 0,
             "ps_debug_gemm32_plan: bad argument");
    const Gemm32Plan p = split_bf16 ? gemm32b_plan(c->tune, R, cin, cout, split_bf16 == 2 ? 1 : 3) : gemm32_plan(c->tune, R, cin, cout);
    out4[0] = p.rw;
    out4[1] = p.cw;
    out4[2] = p.sk;
    out4[3] = p.pd;
    return PS_OK;
}

// --------------------------------------------------------------------------------------------------------
// layer chains on their own (rowgemm.h: rowchain / regchain / rowchain_lds / rowgemm)
// --------------------------------------------------------------------------------------------------------
namespace {

struct ChainBuild {
    PackedLinear L[kChainMaxSteps];
    ChainStep steps[kChainMaxSteps];
    RowSrc s1, s2;
    int n = 0;
};

// the description as ChainStep / RowSrc: the geometry emit() of ps_randla_set_weights gives a layer; the image pointers stay `image` (any non-null
// pointer: the fits / plan functions only test them) until ps_debug_chain has packed them
// (prec: the rule of PS_PREC_BF16 per layer, as pack_images of randla.hip applies it: round iff cin % 16 == 0 and cin >= 32)
int chain_describe(const ps_debug_chain_desc* d, ChainBuild& b, const float* image, bool prec = false)
{
    PS_CHECK(d && d->n_layers >= 1 && d->n_layers <= kChainMaxSteps, "ps_debug_chain: 1..%d layers", kChainMaxSteps);
    PS_CHECK(d->R >= 0 && d->c1 > 0 && d->c2 >= 0 && d->ld1 >= d->c1 && (d->c2 == 0 || d->ld2 >= d->c2), "ps_debug_chain: bad row sources");
    b.n = d->n_layers;
    b.s1.x = d->x1; b.s1.gather = d->g1; b.s1.ld = d->ld1; b.s1.c = d->c1; b.s1.gm = d->g1 ? d->g1m : 0; b.s1.gn = d->g1 ? d->g1n : 0;
    if (d->c2) {
        b.s2.x = d->x2; b.s2.gather = d->g2; b.s2.ld = d->ld2; b.s2.c = d->c2; b.s2.gm = d->g2 ? d->g2m : 0; b.s2.gn = d->g2 ? d->g2n : 0;
    }
    for (int i = 0; i < b.n; ++i) {
        const ps_debug_chain_layer& y = d->layer[i];
        PS_CHECK(y.cin > 0 && y.cout > 0 && y.cin <= 4096 && y.cout <= 4096, "ps_debug_chain: layer %d: bad channel counts", i);
        PS_CHECK(!y.y || y.ldy >= y.cout, "ps_debug_chain: layer %d: ldy below cout", i);
        PS_CHECK(!y.extra || (i > 0 && y.c_extra > 0 && y.ld_extra >= y.c_extra), "ps_debug_chain: layer %d: bad extra source", i);
        PackedLinear& L = b.L[i];
        L = PackedLinear();
        L.cin = y.cin; L.cout = y.cout; L.leaky = y.leaky;
        L.ks = (y.cin + 3) / 4;
        L.ntb = choose_ntb(y.cout);
        L.cblocks = (y.cout + 16 * L.ntb - 1) / (16 * L.ntb);
        L.wp = image; L.bias = image;
        L.round = (prec && y.cin % 16 == 0 && y.cin >= 32) ? 1 : 0;
        ChainStep& st = b.steps[i];
        st = ChainStep();
        st.L = &L; st.y = y.y; st.ldy = y.ldy;
        if (y.extra) {
            st.extra.x = y.extra; st.extra.ld = y.ld_extra; st.extra.c = y.c_extra; st.extra.gather = y.extra_gather;
        }
    }
    return PS_OK;
}

}  // namespace

extern "C" int ps_debug_chain_plan(const ps_debug_chain_desc* d, int* out4)
{
    PS_CHECK(d && out4 && d->R >= 1, "ps_debug_chain_plan: bad argument");
    static const float nothing = 0.f;
    ChainBuild b;
    PS_TRY(chain_describe(d, b, &nothing));
    const ChainPlan p = rowchain_plan(b.steps, b.n, b.s1, b.s2, d->R);
    out4[0] = p.form;
    out4[1] = p.form ? p.blocks : 0;
    out4[2] = p.form ? (int)p.lds_bytes : 0;
    out4[3] = p.fast_in;
    return PS_OK;
}

extern "C" int ps_debug_chain_plan_prec(const ps_debug_chain_desc* d, int precision, int* out4)
{
    PS_CHECK(d && out4 && d->R >= 1 && (precision == 1 || precision == 2), "ps_debug_chain_plan_prec: bad argument");
    static const float nothing = 0.f;
    ChainBuild b;
    PS_TRY(chain_describe(d, b, &nothing, precision == 2));
    const ChainPlan p = rowchain_plan(b.steps, b.n, b.s1, b.s2, d->R);
    out4[0] = p.form;
    out4[1] = p.form ? p.blocks : 0;
    out4[2] = p.form ? (int)p.lds_bytes : 0;
    out4[3] = p.fast_in;
    return PS_OK;
}

extern "C" int ps_debug_chain(ps_context* c, const ps_debug_chain_desc* d, int form)
{
    PS_CHECK(c && d && form >= 0 && form <= 7, "ps_debug_chain: bad argument");
    const bool prec = form >= 4;  // forms 4..7 = forms 0..3 at PS_PREC_BF16
    form &= 3;
    ChainBuild b;
    PS_TRY(chain_describe(d, b, nullptr, prec));
    PS_CHECK(d->x1 && (d->c2 == 0 || d->x2), "ps_debug_chain: NULL row source");
    for (int i = 0; i < b.n; ++i) PS_CHECK(d->layer[i].W, "ps_debug_chain: layer %d has no weights", i);
    if (form == 3) {  // (the chain forms refuse these in their fits tests; layer by layer they would show only after the first layers ran)
        int cur = d->c1 + d->c2;
        for (int i = 0; i < b.n; ++i) {
            const ps_debug_chain_layer& y = d->layer[i];
            PS_CHECK(!(y.extra && y.extra_gather), "ps_debug_chain: layer %d: the extra rows of a chain are plain rows", i);
            cur += y.extra ? y.c_extra : 0;
            PS_CHECK(cur == y.cin, "ps_debug_chain: layer %d expects %d channels, the chain gives %d", i, y.cin, cur);
            cur = y.cout;
        }
    }
    if (d->R == 0) return PS_OK;
    PS_HIP(hipSetDevice(c->device));
    // pack: wp + zero-padded bias (+ the k-permuted image) per layer, one upload; form 3 keeps its un-stored rows behind them
    std::vector<float> host, wround;
    size_t wp_off[kChainMaxSteps], b_off[kChainMaxSteps], wq_off[kChainMaxSteps], tmp_off[kChainMaxSteps];
    auto grow = [&](size_t floats) {
        const size_t off = (host.size() + 63) & ~size_t(63);
        host.resize(off + floats);
        return off;
    };
    for (int i = 0; i < b.n; ++i) {
        const ps_debug_chain_layer& y = d->layer[i];
        PackedLinear& L = b.L[i];
        wp_off[i] = grow(L.packed_floats());
        const float* Wl = y.W;
        if (L.round) {  // a rounded layer: wp of the rounded weights and the direct-load bf16 image instead of the k-permuted one
            wround.resize((size_t)y.cin * y.cout);
            for (size_t t = 0; t < wround.size(); ++t) wround[t] = b3_rounded(y.W[t]);
            Wl = wround.data();
        }
        pack_weights(Wl, y.cin, y.cout, L.ntb, host.data() + wp_off[i]);
        b_off[i] = grow((size_t)L.cout_pad());
        for (int k = 0; k < L.cout_pad(); ++k) host[b_off[i] + k] = (y.bias && k < y.cout) ? y.bias[k] : 0.f;
        wq_off[i] = 0;
        if (L.round) {
            wq_off[i] = grow(L.bf16_bytes() / 4);
            pack_weights_bf16(Wl, y.cin, y.cout, L.ntb, reinterpret_cast<uint16_t*>(host.data() + wq_off[i]));
            continue;
        }
        // (no w32 / w32b / wb image on purpose: form 3 then stays on the 16x16x4 kernels of rowgemm.hip -- the direct-load one for 16-byte aligned
        //  rows of 16-multiple widths, the generic LDS one otherwise -- and never moves to gemm32, which has its own door)
        if (y.cin % 16 == 0) {
            wq_off[i] = grow(L.kperm_floats());
            pack_weights_kperm(y.W, y.cin, y.cout, L.ntb, host.data() + wq_off[i]);
        }
    }
    size_t total = (host.size() + 63) & ~size_t(63);
    for (int i = 0; i < b.n; ++i) {
        tmp_off[i] = total;
        if (form == 3 && !d->layer[i].y) total += ((size_t)d->R * d->layer[i].cout + 63) & ~size_t(63);
    }
    float* dev = nullptr;
    PS_HIP(hipMalloc(reinterpret_cast<void**>(&dev), total * sizeof(float)));
    int rc = PS_OK;
    if (hipMemcpyAsync(dev, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice, c->stream) != hipSuccess) {
        set_error("ps_debug_chain: upload failed");
        rc = PS_EHIP;
    }
    for (int i = 0; i < b.n; ++i) {
        b.L[i].wp = dev + wp_off[i];
        b.L[i].bias = dev + b_off[i];
        if (b.L[i].round) b.L[i].wb = dev + wq_off[i];
        else b.L[i].wq = wq_off[i] ? dev + wq_off[i] : nullptr;
    }
    if (rc == PS_OK) {
        if (form == 0) {
            ChainCache cache;
            if (rowchain_fits(b.steps, b.n, b.s1, b.s2)) rc = rowchain(c, b.steps, b.n, b.s1, b.s2, d->R, &cache);
            else { set_error("ps_debug_chain: the chain fits neither chain kernel (channels above %d, mismatched, or a gathered extra)", kChainMaxC); rc = PS_EINVAL; }
            (void)hipStreamSynchronize(c->stream);
            cache.clear();
        } else if (form == 1) {
            if (regchain_fits(b.steps, b.n, b.s1, b.s2)) rc = regchain(c, b.steps, b.n, b.s1, b.s2, d->R, nullptr);
            else { set_error("ps_debug_chain: not one of regchain's compiled chain shapes"); rc = PS_EINVAL; }
        } else if (form == 2) {
            if (rowchain_lds_plan(b.steps, b.n, b.s1, b.s2, d->R).form == 2) rc = rowchain_lds(c, b.steps, b.n, b.s1, b.s2, d->R);
            else { set_error("ps_debug_chain: the chain does not fit the LDS-staged kernel (channels above %d, mismatched, or a gathered extra)", kChainMaxC); rc = PS_EINVAL; }
        } else {
            RowSrc in1 = b.s1, in2 = b.s2;
            for (int i = 0; i < b.n && rc == PS_OK; ++i) {
                const ChainStep& st = b.steps[i];
                if (i > 0) {
                    in2 = RowSrc();
                    if (st.extra.x) in2 = st.extra;
                }
                float* out = st.y ? st.y : dev + tmp_off[i];
                const int ldo = st.y ? st.ldy : b.L[i].cout;
                rc = rowgemm(c, b.L[i], in1, in2, d->R, out, ldo);
                in1 = RowSrc();
                in1.x = out; in1.ld = ldo; in1.c = b.L[i].cout;
            }
        }
    }
    (void)hipStreamSynchronize(c->stream);
    (void)hipFree(dev);
    return rc;
}

extern "C" int ps_debug_set_regchain_b3(ps_context* c, int on)
{
    PS_CHECK(c && (on == 0 || on == 1), "ps_debug_set_regchain_b3: bad argument");
    c->regchain_b3 = on != 0;
    return PS_OK;
}

extern "C" int ps_debug_set_att_lane(ps_context* c, int on)
{
    PS_CHECK(c && (on == 0 || on == 1), "ps_debug_set_att_lane: bad argument");
    c->att_lane = on != 0;
    return PS_OK;
}

// --------------------------------------------------------------------------------------------------------
// one attentive-pooling stage of a live network (randla_net.h), through each of its stage functions (attpool.h)
// --------------------------------------------------------------------------------------------------------
extern "C" int ps_debug_att_stage(ps_randla* net, int level, int stage, int form, const float* xyz, const int32_t* idx, const int32_t* order,
                                  const float* fg, int64_t n_total, int64_t n_cloud, float* agg)
{
    PS_CHECK(net && xyz && idx && fg && agg, "ps_debug_att_stage: NULL argument");
    PS_CHECK(net->have_weights, "ps_debug_att_stage: weights not set");
    PS_CHECK(level >= 0 && level < net->cfg.num_layers && (stage == 1 || stage == 2) && form >= 0 && form <= 5, "ps_debug_att_stage: bad level / stage / form");
    PS_CHECK(n_total >= 0 && n_cloud >= 1 && n_total % n_cloud == 0, "ps_debug_att_stage: n_total must be a whole number of clouds");
    ps_context* c = net->ctx;
    PS_HIP(hipSetDevice(c->device));
    // form 5, and form 0 of a network at PS_PREC_BF16: that precision's images (packed here when no forward has asked for them yet)
    const bool one_plane = form == 5 || (form == 0 && net->precision == 2);
    const NetImages* images = net;
    if (one_plane && net->enc[level].has_p32) {  // (a level without 32x32 images has no one-plane form: its stage is the default's)
        PS_TRY(randla_bf16_images(net));
        images = net->bf16.get();
    }
    const EncLevel& e = images->enc[level];
    const int d = e.d, h = d / 2;
    const bool use_g = d >= 64;
    AttStage s;
    s.one_plane = one_plane ? 1 : 0;
    s.xyz = xyz; s.idx = idx; s.order = order; s.fg = fg; s.lfa1 = &e.lfa1; s.agg = agg;
    s.n_total = n_total; s.n_cloud = n_cloud; s.d = d; s.k = net->cfg.k_n; s.ldf = use_g ? h + d : h;
    s.p32 = e.has_p32 ? &e.p32 : nullptr;
    s.lfa2 = stage == 2 ? &e.lfa2 : nullptr;
    s.wbot = use_g ? (stage == 1 ? &e.bot1 : &e.bot2) : nullptr;
    s.wfull = use_g ? nullptr : (stage == 1 ? &e.full1 : &e.full2);
    s.lane = stage == 1 ? e.lane1 : e.lane2;
    int rc = PS_EINVAL;
    if (form == 4) rc = att_lane_stage(c, s);  // (refuses everything but d = 16 / K = 16 itself)
    else if (form == 0) rc = att_pool_stage(c, s);
    else if (form == 1 && att_pool32b_fits(s)) rc = att_pool32b_stage(c, s);
    else if (form == 2 && att_pool32_fits(s)) rc = att_pool32_stage(c, s);
    else if (form == 3) rc = att_pool16_stage(c, s);
    else if (form == 5 && att_pool32b_fits(s)) rc = att_pool32b_stage(c, s);
    else set_error("ps_debug_att_stage: the level (d = %d, %lld rows) does not fit the 32x32 form %d", d, (long long)n_total, form);
    (void)hipStreamSynchronize(c->stream);
    return rc;
}

extern "C" int ps_debug_att_form(ps_randla* net, int level, int stage, int k, int64_t n_total)
{
    if (!net || !net->have_weights || level < 0 || level >= net->cfg.num_layers || (stage != 1 && stage != 2) || k < 1 || n_total < 0) {
        set_error("ps_debug_att_form: bad argument");
        return -1;
    }
    const EncLevel& e = net->enc[level];
    const int d = e.d, h = d / 2;
    const bool use_g = d >= 64;
    AttStage s;  // (the fields the dispatch reads, filled as ps_randla_forward fills them)
    s.lfa1 = &e.lfa1; s.lfa2 = stage == 2 ? &e.lfa2 : nullptr;
    s.wbot = use_g ? (stage == 1 ? &e.bot1 : &e.bot2) : nullptr;
    s.wfull = use_g ? nullptr : (stage == 1 ? &e.full1 : &e.full2);
    s.lane = stage == 1 ? e.lane1 : e.lane2;
    s.p32 = e.has_p32 ? &e.p32 : nullptr;
    s.n_total = n_total; s.n_cloud = n_total; s.d = d; s.k = k; s.ldf = use_g ? h + d : h;
    s.one_plane = net->precision == 2 ? 1 : 0;
    return att_pool_form(net->ctx, s);
}

// which: 0 = the level's att_pooling_1 mlp, 1 = its att_pooling_2 mlp, 2 = its [mlp2 ; shortcut], 3 = decoder_0, 4 = decoder step `level`
extern "C" int ps_debug_dense_form(ps_randla* net, int which, int level, int64_t R)
{
    if (!net || !net->have_weights || which < 0 || which > 4 || level < 0 || level >= net->cfg.num_layers || R < 1) {
        set_error("ps_debug_dense_form: bad argument");
        return -1;
    }
    const NetImages* I = net;
    if (net->precision == 2) {
        if (randla_bf16_images(net) != PS_OK) return -1;
        I = net->bf16.get();
    }
    const EncLevel& e = I->enc[level];
    const PackedLinear& L = which == 0 ? e.att1mlp : which == 1 ? e.att2mlp : which == 2 ? e.mlp2sc : which == 3 ? I->decoder0 : I->dec[level];
    static const float4 aligned = {0.f, 0.f, 0.f, 0.f};  // (the fits tests read the alignment of the row pointers, never the rows)
    RowSrc s1, s2;
    s1.x = &aligned.x; s1.c = s1.ld = L.cin;
    if (which == 2) { s1.c = s1.ld = e.d; s2.x = &aligned.x; s2.c = s2.ld = e.d_in; }
    if (which == 4) { s1.c = s1.ld = L.cout; s2.x = &aligned.x; s2.c = s2.ld = L.cin - L.cout; }
    return rowgemm_form(net->ctx, L, s1, s2, R, L.cout);
}

extern "C" int ps_debug_att_lane_pass_points(void) { return att_lane_pass_points(); }

// --------------------------------------------------------------------------------------------------------
// the knobs of struct Tuning (common.h) by field name.  X(field, accepted values of v): the rules of tuning_from_env (context.hip) without
// its clamping -- every field of the struct is listed (tests/test_host_logic.py parses the struct and compares with ps_debug_tuning_fields).
// --------------------------------------------------------------------------------------------------------
static bool is_bool(double v) { return v == 0 || v == 1; }
static bool is_int_in(double v, double lo, double hi) { return v >= lo && v <= hi && v == (double)(int64_t)v; }

#define PS_TUNING_FIELDS(X)                                                \
    X(gemm32b_min_flops, v >= 0 && v <= 1e300)                             \
    X(gemm32b_rw, v == 0 || v == 1 || v == 2)                              \
    X(gemm32b_cw, v == 0 || v == 1 || v == 2)                              \
    X(gemm32_no_sk8, is_bool(v))                                           \
    X(att64_gemm, is_bool(v))                                              \
    X(att64_occ, v == 0 || v == 1 || v == 2)                               \
    X(att_no_split, is_bool(v))                                            \
    X(wgrad_b3_min_rows, is_int_in(v, 0, (double)(1ll << 40)))             \
    X(gemm_b3_min_rows, is_int_in(v, 0, (double)(1ll << 40)))              \
    X(wgrad_wgs, is_int_in(v, 64, 4096))                                   \
    X(bn_slice, is_bool(v))                                                \
    X(inv_bucket, is_bool(v))                                              \
    X(inv_tile, v == 4096 || v == 6144 || v == 8192)                       \
    X(gather_reduce_ordered, is_bool(v))                                   \
    X(maxpool_bwd_ordered, is_bool(v))                                     \
    X(train_act_bf16, is_bool(v))                                          \
    X(train_att_gemm_split, v == -1 || v == 0 || v == 1)                   \
    X(train_att_gemm, is_bool(v))                                          \
    X(train_att128_fwd_gemm, is_bool(v))                                   \
    X(train_fuse_residual, is_bool(v))                                     \
    X(train_merge_syncbn, is_bool(v))                                      \
    X(convbn_max_c, is_int_in(v, 0, 4096))                                 \
    X(convbn_rect_max, is_int_in(v, 0, (double)(1 << 30)))                 \
    X(wgrad_debug, is_bool(v))

extern "C" int ps_debug_set_tuning(ps_context* c, const char* field, double v)
{
    PS_CHECK(c && field, "ps_debug_set_tuning: NULL argument");
#define PS_SET(f, ok)                                                                                 \
    if (std::strcmp(field, #f) == 0) {                                                                \
        PS_CHECK(ok, "ps_debug_set_tuning: %g is not a value %s is compiled for", v, #f);             \
        c->tune.f = static_cast<decltype(c->tune.f)>(v);                                              \
        return PS_OK;                                                                                 \
    }
    PS_TUNING_FIELDS(PS_SET)
#undef PS_SET
    PS_CHECK(false, "ps_debug_set_tuning: no knob named '%s'", field);
}

extern "C" int ps_debug_get_tuning(ps_context* c, const char* field, double* out)
{
    PS_CHECK(c && field && out, "ps_debug_get_tuning: NULL argument");
#define PS_GET(f, ok)                               \
    if (std::strcmp(field, #f) == 0) {              \
        *out = static_cast<double>(c->tune.f);      \
        return PS_OK;                               \
    }
    PS_TUNING_FIELDS(PS_GET)
#undef PS_GET
    PS_CHECK(false, "ps_debug_get_tuning: no knob named '%s'", field);
}

extern "C" int ps_debug_tuning_fields(char* buf, int cap)
{
    static const char names[] =
#define PS_NAME(f, ok) #f "\n"
        PS_TUNING_FIELDS(PS_NAME)
#undef PS_NAME
        ;
    PS_CHECK(buf && cap >= (int)sizeof(names), "ps_debug_tuning_fields: need %d bytes", (int)sizeof(names));
    std::memcpy(buf, names, sizeof(names));
    return PS_OK;
}

// --------------------------------------------------------------------------------------------------------
// white-box door for the GPU test-suite: build one tree on the DEVICE and copy its arrays back (same layout as
// ps_debug_kdtree_host) so the two builders can be compared array for array.
// --------------------------------------------------------------------------------------------------------
extern "C" int ps_debug_kdtree_device(ps_context* c, const float* support, int64_t n, int32_t* vind, int32_t* nodes, float* pts,
                                      int32_t* root_depth, float* bbox)
{
    PS_CHECK(c && support && vind && nodes && pts && root_depth && bbox && n >= 1, "ps_debug_kdtree_device: bad argument");
    PS_HIP(hipSetDevice(c->device));
    PS_TRY(c->stage_in.reserve(sizeof(float) * 3 * (size_t)n));
    PS_HIP(hipMemcpyAsync(c->stage_in.p, support, sizeof(float) * 3 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    TreeSetPlan plan;
    plan.add((int32_t)n);
    for (int pass = 0; pass < 2; ++pass) {
        c->knn_arena.begin(pass == 0);
        plan.carve(c->knn_arena);
        if (pass == 0) PS_TRY(c->knn_arena.buf.reserve(c->knn_arena.off));
    }
    plan.src[0] = c->stage_in.as<float>();
    PS_TRY(build_trees(c, plan));
    int32_t flag[kBuildFlagWords] = {};
    PS_HIP(hipMemcpyAsync(flag, plan.d_flags, sizeof(flag), hipMemcpyDeviceToHost, c->stream));
    PS_HIP(hipStreamSynchronize(c->stream));
    PS_CHECK(flag[kFlagQueueOverflow] == 0, "ps_debug_kdtree_device: builder queue overflow");
    TreeMeta m;
    PS_HIP(hipMemcpyAsync(nodes, plan.d_nodes[0], sizeof(int4) * 2 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    PS_HIP(hipMemcpyAsync(pts, plan.d_pts[0], sizeof(float4) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    PS_HIP(hipMemcpyAsync(&m, plan.d_meta, sizeof(TreeMeta), hipMemcpyDeviceToHost, c->stream));
    PS_HIP(hipStreamSynchronize(c->stream));
    for (int64_t i = 0; i < n; ++i) std::memcpy(&vind[i], &pts[4 * i + 3], 4);
    root_depth[0] = m.root;
    root_depth[1] = m.depth;
    for (int a = 0; a < 3; ++a) {
        bbox[a] = m.lo[a];
        bbox[3 + a] = m.hi[a];
    }
    return PS_OK;
}

// The same for a SET of trees in one plan, as ps_pyramid_build makes them (B clouds x levels), plus the fat image, the copied source
// rows and the builder's counters (debug_hooks.h).
extern "C" int ps_debug_kdtree_device_set(ps_context* c, const float* support, const int32_t* n, int64_t T, const int32_t* want_copy, int32_t* vind,
                                          int32_t* nodes, float* pts, int32_t* fat, int32_t* root_depth, float* bbox, float* copy, int32_t* stats)
{
    PS_CHECK(c && support && n && T >= 1 && vind && nodes && pts && fat && root_depth && bbox && stats, "ps_debug_kdtree_device_set: bad argument");
    size_t tot = 0, tot_copy = 0;
    for (int64_t i = 0; i < T; ++i) {
        PS_CHECK(n[i] >= 1, "ps_debug_kdtree_device_set: tree %lld has %d points", (long long)i, n[i]);
        tot += (size_t)n[i];
        if (want_copy && want_copy[i]) tot_copy += (size_t)n[i];
    }
    PS_CHECK(tot_copy == 0 || copy, "ps_debug_kdtree_device_set: want_copy without a copy buffer");
    PS_HIP(hipSetDevice(c->device));
    PS_TRY(c->stage_in.reserve(sizeof(float) * 3 * tot));
    PS_HIP(hipMemcpyAsync(c->stage_in.p, support, sizeof(float) * 3 * tot, hipMemcpyHostToDevice, c->stream));
    TreeSetPlan plan;
    for (int64_t i = 0; i < T; ++i) plan.add(n[i]);
    float* d_copy = nullptr;
    for (int pass = 0; pass < 2; ++pass) {
        c->knn_arena.begin(pass == 0);
        plan.carve(c->knn_arena);
        d_copy = c->knn_arena.take<float>(3 * tot_copy + 1);
        if (pass == 0) PS_TRY(c->knn_arena.buf.reserve(c->knn_arena.off));
    }
    plan.copy_dst.assign((size_t)T, nullptr);
    {
        size_t off = 0, off_copy = 0;
        for (int64_t i = 0; i < T; ++i) {
            plan.src[i] = c->stage_in.as<float>() + 3 * off;
            off += (size_t)n[i];
            if (want_copy && want_copy[i]) {
                plan.copy_dst[i] = d_copy + 3 * off_copy;
                off_copy += (size_t)n[i];
            }
        }
    }
    PS_TRY(build_trees(c, plan));
    BuildCounters bc;
    PS_TRY(read_build_counters(c, plan, &bc));
    int32_t flag[kBuildFlagWords] = {};
    PS_HIP(hipMemcpyAsync(flag, plan.d_flags, sizeof(flag), hipMemcpyDeviceToHost, c->stream));
    std::vector<TreeMeta> meta((size_t)T);
    PS_HIP(hipMemcpyAsync(meta.data(), plan.d_meta, sizeof(TreeMeta) * (size_t)T, hipMemcpyDeviceToHost, c->stream));
    {
        size_t off = 0;
        for (int64_t i = 0; i < T; ++i) {
            const size_t ni = (size_t)n[i];
            PS_HIP(hipMemcpyAsync(nodes + 4 * 2 * off, plan.d_nodes[i], sizeof(int4) * 2 * ni, hipMemcpyDeviceToHost, c->stream));
            PS_HIP(hipMemcpyAsync(fat + 4 * 6 * off, plan.d_fat[i], sizeof(int4) * 6 * ni, hipMemcpyDeviceToHost, c->stream));
            PS_HIP(hipMemcpyAsync(pts + 4 * off, plan.d_pts[i], sizeof(float4) * ni, hipMemcpyDeviceToHost, c->stream));
            off += ni;
        }
    }
    if (tot_copy) PS_HIP(hipMemcpyAsync(copy, d_copy, sizeof(float) * 3 * tot_copy, hipMemcpyDeviceToHost, c->stream));
    PS_HIP(hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < tot; ++i) std::memcpy(&vind[i], &pts[4 * i + 3], 4);
    for (int64_t i = 0; i < T; ++i) {
        root_depth[2 * i] = meta[(size_t)i].root;
        root_depth[2 * i + 1] = meta[(size_t)i].depth;
        for (int a = 0; a < 3; ++a) {
            bbox[6 * i + a] = meta[(size_t)i].lo[a];
            bbox[6 * i + 3 + a] = meta[(size_t)i].hi[a];
        }
    }
    static_assert(PS_DEBUG_KDTREE_STATS == 6 + 2 * kBuildCounterLevels, "stats layout (debug_hooks.h)");
    stats[0] = bc.chunked_levels;
    for (int l = 0; l < kBuildCounterLevels; ++l) {
        stats[1 + l] = bc.ntasks[l];
        stats[1 + kBuildCounterLevels + l] = bc.nchunks[l];
    }
    stats[1 + 2 * kBuildCounterLevels] = bc.straggler_tasks;
    stats[2 + 2 * kBuildCounterLevels] = bc.mid_pushed;
    stats[3 + 2 * kBuildCounterLevels] = bc.small_pushed;
    stats[4 + 2 * kBuildCounterLevels] = flag[kFlagStackOverflow];
    stats[5 + 2 * kBuildCounterLevels] = flag[kFlagQueueOverflow];
    return PS_OK;
}

// --------------------------------------------------------------------------------------------------------
// the shared primitives on their own: the scan and the radix sort of sortscan.hip (the product library's own code, called through
// sortscan.h) and the partial-sum reducer of reduce_partials.h.  The reducer is a header of templates: the kernels below are the SAME
// text as the product's, instantiated a second time in this library.
// --------------------------------------------------------------------------------------------------------
extern "C" int64_t ps_debug_scan_words(int64_t n) { return n < 0 ? -1 : (int64_t)scan_workspace_words((size_t)n); }
extern "C" int64_t ps_debug_sort_words(int64_t n) { return n < 0 ? -1 : (int64_t)sort_workspace_words((size_t)n); }
extern "C" int ps_debug_scan_launches(int64_t n) { return n < 0 ? -1 : scan_launches((size_t)n); }
extern "C" int ps_debug_sort_launches(int64_t n, int bits) { return n < 0 || bits < 1 || bits > 64 ? -1 : radix_sort_pairs_launches((size_t)n, bits); }

extern "C" int ps_debug_scan_u32(ps_context* c, const uint32_t* in, uint32_t* out, int64_t n, uint32_t* work)
{
    PS_CHECK(c && in && out && work && n >= 0, "ps_debug_scan_u32: bad argument");
    PS_HIP(hipSetDevice(c->device));
    exclusive_scan_u32(c->stream, in, out, (size_t)n, work);
    PS_HIP(hipGetLastError());
    PS_HIP(hipStreamSynchronize(c->stream));
    return PS_OK;
}

extern "C" int ps_debug_sort_pairs(ps_context* c, int key_bytes, void* k0, void* k1, uint32_t* v0, uint32_t* v1, int64_t n, int bits, uint32_t* work,
                                   int* which_out)
{
    PS_CHECK(c && k0 && k1 && v0 && v1 && work && which_out && n >= 0, "ps_debug_sort_pairs: bad argument");
    PS_CHECK(key_bytes == 4 || key_bytes == 8, "ps_debug_sort_pairs: key_bytes must be 4 or 8");
    PS_CHECK(bits >= 1 && bits <= 8 * key_bytes, "ps_debug_sort_pairs: bits must be 1..%d", 8 * key_bytes);
    PS_HIP(hipSetDevice(c->device));
    *which_out = key_bytes == 4
                     ? radix_sort_pairs_u32(c->stream, static_cast<unsigned*>(k0), static_cast<unsigned*>(k1), v0, v1, (size_t)n, bits, work)
                     : radix_sort_pairs_u64(c->stream, static_cast<unsigned long long*>(k0), static_cast<unsigned long long*>(k1), v0, v1, (size_t)n,
                                            bits, work);
    PS_HIP(hipGetLastError());
    PS_HIP(hipStreamSynchronize(c->stream));
    return PS_OK;
}

extern "C" int ps_debug_reduce_partials(ps_context* c, int form, const void* part, int n_part, int nv, int n0, void* out0, void* out1)
{
    PS_CHECK(c && part && out0 && n_part >= 0 && nv >= 0 && form >= 0 && form <= 3, "ps_debug_reduce_partials: bad argument");
    PS_CHECK(form < 2 || (out1 && n0 >= 0 && n0 <= nv), "ps_debug_reduce_partials: forms 2 and 3 need out1 and 0 <= n0 <= nv");
    PS_HIP(hipSetDevice(c->device));
    if (nv == 0) return PS_OK;
    const dim3 grid((unsigned)((nv + 15) / 16)), block(256);  // the grid of every caller
    switch (form) {
    case 0:
        hipLaunchKernelGGL(reduce_partials_kernel<float>, grid, block, 0, c->stream, static_cast<const float*>(part), n_part, nv, static_cast<float*>(out0));
        break;
    case 1:
        hipLaunchKernelGGL(reduce_partials_kernel<double>, grid, block, 0, c->stream, static_cast<const double*>(part), n_part, nv,
                           static_cast<double*>(out0));
        break;
    case 2:
        hipLaunchKernelGGL((reduce_partials2_kernel<float>), grid, block, 0, c->stream, static_cast<const float*>(part), n_part, nv, n0,
                           static_cast<float*>(out0), static_cast<float*>(out1));
        break;
    default:
        hipLaunchKernelGGL((reduce_partials2_kernel<float, double>), grid, block, 0, c->stream, static_cast<const float*>(part), n_part, nv, n0,
                           static_cast<float*>(out0), static_cast<float*>(out1));
        break;
    }
    PS_HIP(hipGetLastError());
    PS_HIP(hipStreamSynchronize(c->stream));
    return PS_OK;
}
