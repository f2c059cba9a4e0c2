#!/usr/bin/env python3
"""Generates tests/golden/saliency_mixup.npz (run in the BUILD container only, like make_saliency_data_golden.py): the REAL mixup of the
reference, cut out of SaliencyAttention/utils.py:511-527 with ast (the module itself needs nibabel / SimpleITK) and run UNMODIFIED on
small float32 samples.  np.random.beta is patched to hand back chosen gammas (and asserts that it was asked for Beta(0.4, 0.4)).  Only the
resulting arrays are committed.

    python tests/golden/make_saliency_mixup_golden.py <root of the reference repository>
"""
import ast
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1]
GAMMAS = (0.0, 1.0, 0.5, 1.0 - 2.0 ** -30, 1e-12, 0.34029683942911143)


def cut(path, names):
    out = {}
    for node in ast.walk(ast.parse(open(path).read())):
        if isinstance(node, ast.FunctionDef) and node.name in names:
            out[node.name] = ast.Module(body=[node], type_ignores=[])
    assert set(out) == set(names), (path, sorted(out))
    return out


env = dict(np=np)
for name, mod in cut(os.path.join(REF, "SaliencyAttention/utils.py"), ("mixup",)).items():
    exec(compile(mod, "utils.py", "exec"), env)

real_beta = np.random.beta
out = {"gammas": np.array(GAMMAS, np.float64), "classes": np.array([2, 4], np.int64)}
rng = np.random.default_rng(511)
for K in (2, 4):
    n = 320
    samples = []
    for _ in range(2):
        image = (rng.integers(-4000, 4000, n).astype(np.float32) / 7).astype(np.float32)  # inexact in float32: the products round
        image[rng.random(n) < 0.15] = 0
        weight = (rng.random(n) < 0.6).astype(np.float32)
        label = rng.integers(0, K, n)
        hot = np.eye(K, dtype=np.float32)[label]  # data_sampler.py:329-337: one-hot before batching
        samples.append([image, weight, hot])
    assert (samples[0][0] < 0).any() and (samples[0][0] == 0).any() and ((samples[0][1] == 0) & (samples[1][1] == 0)).any()
    out.update({"image_a%d" % K: samples[0][0], "weight_a%d" % K: samples[0][1], "hot_a%d" % K: samples[0][2],
                "image_b%d" % K: samples[1][0], "weight_b%d" % K: samples[1][1], "hot_b%d" % K: samples[1][2]})
    for i, gamma in enumerate(GAMMAS):
        def beta(a, b, gamma=gamma):
            assert (a, b) == (0.4, 0.4)
            return gamma
        np.random.beta = beta
        try:
            image, weight, hot = env["mixup"](samples[0], samples[1])
        finally:
            np.random.beta = real_beta
        assert image.dtype == np.float32 and hot.dtype == np.float32 and weight.dtype == np.bool_
        out.update({"mix_image%d_%d" % (K, i): image, "mix_weight%d_%d" % (K, i): weight, "mix_hot%d_%d" % (K, i): hot})

path = os.path.join(HERE, "saliency_mixup.npz")
np.savez_compressed(path, **out)
print("saliency_mixup.npz", os.path.getsize(path))
assert os.path.getsize(path) < 300 * 1024
