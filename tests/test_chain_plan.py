"""Which kernel every layer chain of the forward resolves to (csrc/rowgemm.h: rowchain), through the host-only door ps_debug_chain_plan: the
chains of the shipped configurations must all be regchain's compiled shapes -- a configuration change that silently moved one onto the slower
LDS-staged kernel (or off the chains altogether) shows up here, without a GPU."""
from test_gpu_forward_stages import bind, plan, shape_desc


def _network_chains(in_channels, num_classes, d_out):
    """The chains ps_randla_forward tries (csrc/randla.hip), in launch order: (name, [(cin, cout)], c1, c2, extras).  A hand-kept mirror:
    it must follow the forward's launch plan when that changes.  One difference: below d = 64 the forward takes a one-step chain only when
    regchain fits (otherwise rowgemm), while the plan door would report the LDS form for it -- the tests here assert form 1 or 0 for those."""
    out = [("fc0+mlp1", [(in_channels, 8), (8, d_out[0] // 2)], in_channels, 0, None)]
    d_in = 8
    for i, d in enumerate(d_out):
        h = d // 2
        g = [(h, d)] if d >= 64 else []  # the score pre-product G = f . Wfc[:h] rides on the chain from d = 64
        if i > 0:
            out.append(("enc%d mlp1" % i, [(d_in, h)] + g, d_in, 0, None))
        out.append(("enc%d att1-mlp" % i, [(d, h)] + g, d, 0, None))
        out.append(("enc%d att2-mlp+mlp2+shortcut" % i, [(d, d), (d + d_in, 2 * d)], d, 0, {1: d_in}))
        d_in = 2 * d
    c = 2 * d_out[0]
    out.append(("head", [(2 * c, c), (c, 64), (64, 32), (32, num_classes)], c, c, None))
    return out


def _forms(dbg, chains, R=45000):
    return {name: plan(dbg, shape_desc(layers, c1, c2, R=R, extras=extras))[0] for name, layers, c1, c2, extras in chains}


def test_shipped_configurations_run_every_chain_on_regchain(dbg):
    from point_unet_amd.helper_tool import ConfigBraTS, ConfigPancreas
    bind(dbg)
    for cfg in (ConfigBraTS, ConfigPancreas):
        forms = _forms(dbg, _network_chains(cfg.in_channels, cfg.num_classes, list(cfg.d_out)[:cfg.num_layers]))
        chained = sorted(n for n, f in forms.items() if f)
        # levels 0-1 entirely, level 2's two feature chains (its last pair is 256 channels wide), and the head; deeper levels run one GEMM per layer
        assert chained == sorted(["fc0+mlp1", "enc0 att1-mlp", "enc0 att2-mlp+mlp2+shortcut", "enc1 mlp1", "enc1 att1-mlp", "enc1 att2-mlp+mlp2+shortcut",
                                  "enc2 mlp1", "enc2 att1-mlp", "head"]), forms
        assert all(forms[n] == 1 for n in chained), forms


def test_a_first_level_of_32_channels_takes_the_lds_form(dbg):
    bind(dbg)
    forms = _forms(dbg, _network_chains(7, 4, [32, 64]))
    assert forms["fc0+mlp1"] == 1                      # 7 -> 8 -> 16: still one tile per layer
    assert forms["enc0 att2-mlp+mlp2+shortcut"] == 2   # 32 -> 32, [32 | 8] -> 64: not a compiled shape
    assert forms["head"] == 0                          # [64 | 64] -> 64 is 128 inputs wide: above kChainMaxC, one GEMM per layer


def test_plan_reports_the_launch(dbg):
    """Workgroups follow the rows up to the cap (256 CUs x workgroups that fit a CU's 160 KB of LDS, at most 4); the LDS form reports its staging."""
    bind(dbg)
    fc0 = [(7, 8), (8, 8)]
    assert plan(dbg, shape_desc(fc0, 7, R=1))[:2] == (1, 1)
    assert plan(dbg, shape_desc(fc0, 7, R=65))[:2] == (1, 2)
    assert plan(dbg, shape_desc(fc0, 7, R=1 << 22))[:2] == (1, 1024)
    form, blocks, lds, fast_in = plan(dbg, shape_desc([(32, 24), (24, 16)], 32, R=1 << 22))
    assert form == 2 and blocks == 256 * min(4, 160 * 1024 // lds) and fast_in == 3
    assert plan(dbg, shape_desc([(32, 24), (24, 16)], 32, R=100, ld1=33))[3] == 0
    assert plan(dbg, shape_desc([(100, 16)], 100, R=100))[0] == 0  # above kChainMaxC
