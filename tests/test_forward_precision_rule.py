"""include/pointseg_forward_precision.h without a GPU: the restated rule (tests/forward_precision_ref.py) names the layers the header
names, the rounding is round-to-nearest-even, and on every attention case of tests/test_gpu_forward_precision.py the rounding model's own
float32 noise is small against the bfloat16 effect the GPU test measures against."""
import numpy as np
import pytest

import forward_precision_ref as ref
from point_unet_amd import weights
from point_unet_amd.helper_tool import ConfigBraTS, ConfigPancreas

T, F = True, False
# per level: mlp1, LocSE (LFAmlp1), att_pooling_1 fc, att_pooling_1 mlp, LFA mlp2, att_pooling_2 fc, att_pooling_2 mlp, mlp2, shortcut
# as (K axis, rounded); mlp2 and shortcut are one product over d + d_in
_LEVELS = [
    [(8, F), (10, F), (16, F), (16, F), (8, F), (16, F), (16, F), (24, F), (24, F)],                      # d = 16: nothing
    [(32, T), (10, F), (64, T), (64, T), (32, T), (64, T), (64, T), (96, T), (96, T)],                    # d = 64
    [(128, T), (10, F), (128, T), (128, T), (64, T), (128, T), (128, T), (256, T), (256, T)],             # d = 128
    [(256, T), (10, F), (256, T), (256, T), (128, T), (256, T), (256, T), (512, T), (512, T)],            # d = 256
    [(512, T), (10, F), (512, T), (512, T), (256, T), (512, T), (512, T), (1024, T), (1024, T)],          # d = 512
]
_TAIL = [(1024, T), (1536, T), (768, T), (384, T), (160, T), (64, T), (32, T), (64, T), (32, T)]  # decoder_0, five decoder steps, fc1, fc2, fc


@pytest.mark.parametrize("cfg", [ConfigBraTS, ConfigPancreas])
def test_the_rule_on_the_two_models(cfg):
    want = [(cfg.in_channels, F)] + [e for lvl in _LEVELS for e in lvl] + _TAIL
    got = ref.rule_table(cfg)
    assert [s for s, _, _ in got] == [s for s, _, _, _ in weights.layer_dims(cfg)]
    assert [(k, r) for _, k, r in got] == want
    by = {s: r for s, _, r in got}
    assert not by["fc0"] and not any(r for s, r in by.items() if s.startswith("Encoder_layer_0"))
    assert not any(r for s, r in by.items() if s.endswith("LFAmlp1"))
    assert all(r for s, r in by.items() if s != "fc0" and not s.startswith("Encoder_layer_0") and not s.endswith("LFAmlp1"))


def test_rb_is_round_to_nearest_even():
    bits = np.array([0x3F800000, 0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0xBF808000, 0xBF818000, 0x3F80FFFF, 0x00000000], np.uint32)
    x = bits.view(np.float32)
    want = np.array([0x3F800000, 0x3F800000, 0x3F820000, 0x3F810000, 0x3F800000, 0xBF800000, 0xBF820000, 0x3F810000, 0x00000000], np.uint32)
    assert np.array_equal(ref.rb(x).view(np.uint32), want)  # ties (.8000) go to the even neighbour, both signs
    assert not np.array_equal(ref.rb(x), ref.truncate(x))
    assert np.array_equal(ref.truncate(x).view(np.uint32), bits & np.uint32(0xFFFF0000))
    assert np.array_equal(ref.rb(ref.rb(x)), ref.rb(x))
    x64 = x.astype(np.float64)
    assert ref.rb(x64).dtype == np.float64 and np.array_equal(ref.rb(x64), ref.rb(x).astype(np.float64))


def test_the_unrounded_model_is_the_oracle():
    """The restated graph with no rounding is oracle/randla_oracle.py's inference up to the float32 folding of the weights."""
    from oracle import randla_oracle as ro

    class Cfg:
        k_n, num_layers, num_classes, in_channels = 16, 2, 4, 7
        sub_sampling_ratio = [4, 4]
        d_out = [16, 64]

    rng = np.random.default_rng(3)
    xyz = rng.random((1, 256, 3), dtype=np.float32)
    feats = np.concatenate([xyz, rng.standard_normal((1, 256, 4)).astype(np.float32)], -1)

    def knn(s, q, k):
        d2 = ((q[:, :, None, :] - s[:, None, :, :]) ** 2).sum(-1)
        return np.argsort(d2, axis=-1, kind="stable")[:, :, :k]

    pts, nbr, pool, up = ro.build_pyramid(knn, xyz, Cfg.k_n, Cfg.sub_sampling_ratio)
    p = weights.init_params(Cfg, seed=2, randomize_bn=True)
    want = ro.inference(p, Cfg.num_layers, pts, nbr, pool, up, feats, np.float64)
    got = ref.inference(Cfg, p, pts, nbr, pool, up, feats, np.float64, rounded=False)
    assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max()
    model = ref.inference(Cfg, p, pts, nbr, pool, up, feats, np.float64)
    dist = np.abs(model - want).max()
    assert 1e-4 * np.abs(want).max() < dist < 5e-2 * np.abs(want).max()  # a bfloat16-class effect, and there is one


_PARAMS = {}


def _params(d, K):
    if (d, K) not in _PARAMS:
        _PARAMS[(d, K)] = weights.init_params(ref.OneLevel(d, K), seed=d + K, randomize_bn=True)  # (test_gpu_forward_stages._net's parameters)
    return _PARAMS[(d, K)]


@pytest.mark.parametrize("d", [64, 128, 256, 512])
def test_the_models_float32_noise_is_a_40th_of_the_bf16_effect(d):
    """Every attention case of the GPU test: max |model32 - model64| <= 0.025 dist, which makes the GPU bar of 0.1 dist a 4 x margin over
    the reference's own noise.  Seeds: ref.att_cases.  The second-tile walks repeat a geometry pattern of ref.PERIOD points under random
    features (ref.att_case): on a random cloud of 4 133 x 32 x h operands no seed keeps the reference clear of bfloat16 boundaries.
    (Stage 1 of a level of ONE point has K equal rows, a uniform softmax whatever the scores are, and dist = 0 exactly: there, and only
    there, the bound is ref.FP32_FLOOR, the fp32 error of the arithmetic the contract does not round.)"""
    worst = 0.0
    for dd, K, stage, B, n, seed, period in ref.att_cases():
        if dd != d:
            continue
        _, _, _, exact64, model64, model32 = ref.att_case(_params(d, K), d, K, stage, B, n, seed, period)
        dist = float(np.abs(exact64 - model64).max())
        flip = float(np.abs(model32.astype(np.float64) - model64).max())
        what = "d %d K %d stage %d %d x %d seed %d: flip spread %.3e, dist %.3e" % (d, K, stage, B, n, seed, flip, dist)
        if B * n == 1 and stage == 1:
            assert dist == 0 and flip <= ref.FP32_FLOOR * float(np.abs(exact64).max()), what
            continue
        assert dist > 1e-5 * float(np.abs(exact64).max()), what
        worst = max(worst, flip / dist)
        assert flip <= 0.025 * dist, what
    print("d %d: largest flip spread / dist = %.3e" % (d, worst))
