"""The kernels of include/pointseg_saliency_data.h and the Python surface over them (point_unet_amd.saliency_data): the preparation against
the reference's own functions (tests/golden/saliency_data.npz) and the numpy restatement, the patch sampler against the restatement bit for
bit -- every output between guard bands --, PatchBank, train_saliency against the same steps written out by hand, evaluate_saliency against
binary_dice3d in numpy."""
import ctypes
import os

import numpy as np
import pytest

import saliency_data_ref as ref

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAND = 4096
MODE_ID = {"random": 0, "all_positive": 1, "one_positive": 2}


def _sd():
    from point_unet_amd import saliency_data
    return saliency_data


def _np(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "saliency_data.npz"))


# ---- preparation ---------------------------------------------------------------------------------------------------------------------------

def _check_brats(bank, c, want, tol_of):
    image, label, weight = bank.whole(c)
    assert bank.bbox(c) == (want["box"][0], want["box"][1]) and bank.shape(c) == want["label"].shape
    assert image.dtype == torch.float32 and label.dtype == torch.uint8 and weight.dtype == torch.uint8
    assert np.array_equal(_np(weight), want["weight"]) and np.array_equal(_np(label), want["label"])
    got = np.moveaxis(_np(image), 0, -1).astype(np.float64)
    err = float(np.abs(got - tol_of).max())
    print("z-score: max |difference| %.3e, bar %.3e" % (err, 2e-7 * np.abs(tol_of).max()))
    assert got.shape == tol_of.shape and err <= 2e-7 * np.abs(tol_of).max()
    assert np.array_equal(got == 0, want["image"] == 0) and np.isfinite(got).all()


def test_brats_preparation_against_the_reference_functions(golden):
    """Box, weight and labels exact; the z-score within 2e-7 max|x| of the reference's (float64 sums in another order, then one cast)."""
    g = golden
    bank = _sd().PatchBank(4)
    for num_class, key in ((4, "label4"), (2, "label2")):
        c = bank.add_brats(g["raw"], g["seg"], num_class=num_class, margin=int(g["margin"]))
        want = {"box": (g["bbmin"].tolist(), g["bbmax"].tolist()), "label": g[key].astype(np.uint8), "weight": g["weight"].astype(np.uint8),
                "image": np.moveaxis(g["normalised"], 0, -1)}
        _check_brats(bank, c, want, np.moveaxis(g["normalised"], 0, -1).astype(np.float64))
    c = bank.add_brats(torch.from_numpy(g["raw"]).cuda())  # a CUDA tensor, no segmentation: the same crop, labels 0
    assert bank.bbox(c) == bank.bbox(0) and int(bank.whole(c)[1].max()) == 0 and torch.equal(bank.whole(c)[0], bank.whole(1)[0])
    assert len(bank) == 3


def test_brats_preparation_refuses_what_cannot_be_normalised(golden):
    from point_unet_amd import PointSegError
    bank = _sd().PatchBank(4)
    raw = golden["raw"].copy()
    with pytest.raises(PointSegError, match="raw\\[0\\] is all zero"):
        bank.add_brats(np.concatenate([np.zeros_like(raw[:1]), raw[1:]]))
    raw[2] = -np.abs(raw[2])
    with pytest.raises(PointSegError, match="modality 2 has no voxel above zero"):
        bank.add_brats(raw)
    raw[2] = np.where(raw[2] != 0, 1.0, 0.0)
    raw[2, 0, 6, 6] = 1.0
    with pytest.raises(PointSegError, match="modality 2 has mean 1 and std 0"):
        bank.add_brats(raw)
    assert len(bank) == 0
    assert bank.add_brats(golden["raw"]) == 0  # the bank still works


def test_brats_preparation_of_a_volume_of_many_workgroups():
    """(40, 48, 52), two modalities: 25 slabs of 4096 crop voxels per modality; against the numpy restatement, twice with the same bits."""
    rng = np.random.default_rng(3)
    shape = (40, 48, 52)
    raw = rng.normal(50, 40, (2,) + shape).astype(np.float32)
    raw[:, rng.random(shape) < 0.2] = 0
    raw[0, :3], raw[0, :, :9], raw[0, :, :, 47:] = 0, 0, 0  # the box: [0 (clamped), 39] x [4, 47] x [0, 51 (clamped)]
    seg = rng.choice([0, 1, 2, 4], shape).astype(np.int32)
    want = ref.brats_prepare(raw, seg, 4, 5)
    assert want["box"] == ([0, 4, 0], [39, 47, 51])
    bank = _sd().PatchBank(2)
    a, b = bank.add_brats(raw, seg, num_class=4), bank.add_brats(raw, seg.astype(np.int64), num_class=4)
    _check_brats(bank, a, want, want["image"].astype(np.float64))
    assert torch.equal(bank.whole(a)[0], bank.whole(b)[0])


def test_pancreas_preparation_bit_for_bit(golden):
    g = golden
    bank = _sd().PatchBank(1)
    label = (g["ct"] > 0).astype(np.uint8) * 3
    a = bank.add_pancreas(g["ct"], label)
    b = bank.add_pancreas(g["ct"].astype(np.float32))
    image, lab, weight = bank.whole(a)
    assert image.shape == (1,) + g["ct"].shape and np.array_equal(_np(image)[0], g["ct_rescaled"].astype(np.float32))
    assert np.array_equal(_np(lab), label) and int(weight.min()) == 1 == int(weight.max())
    assert torch.equal(bank.whole(b)[0], image) and int(bank.whole(b)[1].max()) == 0
    assert bank.bbox(a) == ([0, 0, 0], [5, 6, 7]) and bank.shape(a) == (6, 7, 8)
    want = ref.pancreas_prepare(g["ct"], label)
    assert np.array_equal(_np(image)[0], want["image"][..., 0])


# ---- the sampler against the restatement ---------------------------------------------------------------------------------------------------

def _make_bank(C, shapes, seed, ctx=None):
    """Per shape one volume with labels (30 % positive) and one without any: volumes 0 .. n-1 and n .. 2n-1.  (numpy volumes, PatchBank)"""
    rng = np.random.default_rng(seed)
    vols = []
    for empty in (False, True):
        for s in shapes:
            label = np.zeros(s, np.uint8) if empty else ((rng.random(s) < 0.3) * rng.integers(1, 4, s)).astype(np.uint8)
            if not empty:
                label[tuple(d // 2 for d in s)] = 2  # (a volume smaller than the patch is copied whole: its windows are never empty)
            vols.append({"image": rng.standard_normal(s + (C,)).astype(np.float32), "label": label, "weight": (rng.random(s) < 0.7).astype(np.uint8)})
    bank = _sd().PatchBank(C, ctx=ctx)
    for v in vols:
        bank.add_prepared(v["image"], v["label"], v["weight"])
    return vols, bank


def _banded(nbytes, shift):
    """nbytes of device memory, `shift` bytes past a 256-byte boundary, between two bands of 0xA5."""
    buf = torch.full((BAND + shift + nbytes + BAND,), 0xA5, dtype=torch.uint8, device="cuda")
    return buf, buf[BAND + shift:BAND + shift + nbytes]


def _direct(bank, cand, P, seed, mode, shift=0, bad=None):
    """ps_patch_sample itself, every output between guard bands.  Returns (rc, outputs as numpy, True when every band is intact, the raw
    output bytes)."""
    from point_unet_amd import _lib, runtime
    cand = np.ascontiguousarray(cand, dtype=np.int32)
    B, T = cand.shape
    V = int(np.prod(P))
    C = bank.channels
    shapes = {"images": ((B,) + tuple(P) + (C,), torch.float32), "weights": ((B,) + tuple(P), torch.float32), "labels": ((B,) + tuple(P), torch.int32),
              "info": ((B, 8), torch.int32)}
    bufs = {k: _banded(4 * int(np.prod(s)), shift) for k, (s, _) in shapes.items()}
    images, labels, weights, dims, n = bank.c_tables()
    bank.ctx.use_torch_stream()
    a = dict(ctx=bank.ctx.handle, images=images, labels=labels, weights=weights, dims=dims, n=n, C=C, cand=cand.ctypes.data_as(_lib.c_i32p), B=B, T=T,
             P=(ctypes.c_int64 * 3)(*P), seed=seed, mode=MODE_ID[mode], oi=runtime.ptr(bufs["images"][1]), ow=runtime.ptr(bufs["weights"][1]),
             ol=runtime.ptr(bufs["labels"][1]), oinfo=runtime.ptr(bufs["info"][1]))
    a.update(bad or {})
    rc = _lib.lib().ps_patch_sample(*a.values())
    torch.cuda.synchronize()
    intact = all(bool((full[:BAND + shift] == 0xA5).all()) and bool((full[BAND + shift + part.numel():] == 0xA5).all()) for full, part in bufs.values())
    raw = {k: _np(part).copy() for k, (_, part) in bufs.items()}
    outs = {k: raw[k].view(np.float32 if dt == torch.float32 else np.int32).reshape(s) for k, (s, dt) in shapes.items()}
    assert V > 0
    return rc, outs, intact, raw


def _equal_to_the_rule(vols, bank, cand, P, seed, mode, shift=0):
    rc, got, intact, _ = _direct(bank, cand, P, seed, mode, shift)
    from point_unet_amd import _lib
    assert rc == 0, _lib.lib().ps_last_error()
    images, weights, labels, info = ref.sample(vols, cand, P, seed, mode)
    assert np.array_equal(got["info"], info), (got["info"], info)
    assert np.array_equal(got["labels"], labels) and np.array_equal(got["weights"], weights)
    assert np.array_equal(got["images"].view(np.uint32), images.view(np.uint32))
    assert intact, "a guard band was written"
    return info


def _cands(n, B, T):
    """Candidate tables over the bank of _make_bank (labelled volumes 0 .. n-1, empty ones n .. 2n-1), by the branch they take."""
    lab = lambda i: i % n
    emp = lambda i: n + i % n
    mixed = np.array([[lab(b + t) if (b + t) % 2 == 0 else emp(b + t) for t in range(T)] for b in range(B)])
    same = np.full((B, T), lab(1))                                  # the same volume in every slot and try
    none = np.array([[emp(b + 2 * t) for t in range(T)] for b in range(B)])
    late = none.copy()
    late[B - 1, T - 1] = lab(0)                                     # only the last try of the last slot is positive
    late_all = none.copy()
    late_all[:, T - 1] = [lab(b) for b in range(B)]                 # every slot's last try (all_positive)
    first = none.copy()
    first[0, 0] = lab(2)                                            # an earlier slot is positive (B > 1)
    return {"mixed": mixed, "same": same, "none": none, "late": late, "late_all": late_all, "first": first}


CASES = [
    # (C, patch, volume shapes): odd offsets, P2 * C no multiple of 4 (C = 1) and a multiple of 4 at odd offsets (C = 4)
    (1, (5, 6, 7), ((9, 20, 23), (4, 6, 30), (5, 6, 7))),
    (4, (5, 6, 7), ((9, 20, 23), (4, 6, 30), (5, 6, 7))),
    # nearly all fill
    (1, (8, 8, 8), ((2, 3, 3), (1, 1, 1))),
    (4, (8, 8, 8), ((2, 3, 3), (1, 1, 1))),
    # the aligned fast path and one past it
    (1, (16, 16, 16), ((16, 16, 16), (17, 33, 19))),
    (4, (16, 16, 16), ((16, 16, 16), (17, 33, 19))),
]


@pytest.mark.parametrize("C, P, shapes", CASES, ids=["C%d-P%d-%s" % (c, p[0], "x".join(map(str, s[0]))) for c, p, s in CASES])
def test_sampler_equals_the_rule_bit_for_bit(C, P, shapes):
    vols, bank = _make_bank(C, shapes, seed=100 + C + P[0])
    n = len(shapes)
    seen = set()
    for B in (1, 3):
        for T in (1, 4):
            cands = _cands(n, B, T)
            for mode in ref.MODES:
                for name in ("mixed", "same", "none", "late", "late_all", "first"):
                    if B * T == 1 and name not in ("mixed", "none"):
                        continue
                    info = _equal_to_the_rule(vols, bank, cands[name], P, 7 + 13 * B + T, mode)
                    seen.add((mode, name, B, T, tuple(info[:, 0]), tuple(info[:, 6])))
    tries = lambda mode, name, B=3, T=4: [(s[4], s[5]) for s in seen if s[:4] == (mode, name, B, T)][0]
    # each branch of the choice was taken
    assert tries("one_positive", "none") == ((0, 0, 3), (1, 1, 0)) and tries("all_positive", "none") == ((3, 3, 3), (0, 0, 0))
    assert tries("random", "none") == ((0, 0, 0), (1, 1, 1)) and tries("random", "same") == ((0, 0, 0), (1, 1, 1))
    assert tries("one_positive", "late") == ((0, 0, 3), (1, 1, 1)) and tries("all_positive", "late_all") == ((3, 3, 3), (1, 1, 1))
    assert tries("one_positive", "first") == ((0, 0, 0), (1, 1, 1)) and tries("all_positive", "first") == ((0, 3, 3), (1, 0, 0))
    assert tries("one_positive", "none", 1, 4) == ((3,), (0,)) and tries("one_positive", "none", 3, 1) == ((0, 0, 0), (1, 1, 0))
    # outputs that are not 16-byte aligned take the scalar stores: the same bytes
    cands = _cands(n, 3, 4)
    for mode, name in (("one_positive", "mixed"), ("all_positive", "late_all")):
        _equal_to_the_rule(vols, bank, cands[name], P, 5, mode, shift=4)


def test_sampler_is_deterministic_across_calls_contexts_and_streams():
    from point_unet_amd import runtime
    shapes = ((9, 20, 23), (17, 33, 19))
    vols, bank = _make_bank(4, shapes, seed=1)
    _, bank2 = _make_bank(4, shapes, seed=1, ctx=runtime.default_context(0))
    cand = _cands(2, 3, 4)["mixed"]
    torch.cuda.synchronize()
    first = bank.sample(cand, (5, 6, 7), seed=21)
    again = bank.sample(cand, (5, 6, 7), seed=21)
    other = bank2.sample(cand, (5, 6, 7), seed=21)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        private = bank.sample(cand, (5, 6, 7), seed=21)
    torch.cuda.synchronize()
    for k in ("images", "weights", "labels", "info"):
        for o in (again, other, private):
            assert torch.equal(first[k].view(torch.int32), o[k].view(torch.int32)), k
    moved = bank.sample(cand, (5, 6, 7), seed=22)
    assert not torch.equal(first["info"], moved["info"])


def test_argument_errors_leave_the_outputs_untouched():
    from point_unet_amd import _lib
    vols, bank = _make_bank(1, ((9, 20, 23),), seed=2)
    good = np.array([[0, 1], [1, 0]])
    err = _lib.lib().ps_last_error
    for kw, word in ((dict(B=65), b"B = 65"), (dict(T=0), b"T = 0"), (dict(C=17), b"C = 17"), (dict(mode=5), b"mode = 5"), (dict(n=1), b"cand[0, 1] = 1"),
                     (dict(P=(ctypes.c_int64 * 3)(5, 0, 7)), b"P = [5, 0, 7]"), (dict(ow=None), b"NULL out_images"), (dict(images=None), b"NULL images"),
                     (dict(dims=(ctypes.c_int64 * 6)(9, 20, 23, 9, 20, 0)), b"dims of volume 1")):
        rc, _, intact, raw = _direct(bank, good, (5, 6, 7), 3, "one_positive", bad=kw)
        assert rc == 1 and word in err(), (kw, err())
        assert intact and all(bool((v == 0xA5).all()) for v in raw.values()), kw
    rc, _, intact, raw = _direct(bank, np.array([[0, 2], [1, 0]]), (5, 6, 7), 3, "one_positive")
    assert rc == 1 and b"cand[0, 1] = 2" in err() and intact and all(bool((v == 0xA5).all()) for v in raw.values())
    rc, _, intact, _ = _direct(bank, good, (5, 6, 7), 3, "one_positive")
    assert rc == 0 and intact


# ---- PatchBank -----------------------------------------------------------------------------------------------------------------------------

def test_patch_bank_sample_epoch_batches_and_whole():
    sd = _sd()
    shapes = ((9, 20, 23), (4, 6, 30), (5, 6, 7), (8, 9, 10))
    vols, bank = _make_bank(1, shapes, seed=4)  # 8 volumes
    assert len(bank) == 8
    for mode in ref.MODES:
        cand = _cands(4, 3, 4)["mixed"]
        got = bank.sample(cand, (5, 6, 7), seed=31, mode=mode)
        images, weights, labels, info = ref.sample(vols, cand, (5, 6, 7), 31, mode)
        assert np.array_equal(_np(got["images"]), images) and np.array_equal(_np(got["weights"]), weights)
        assert np.array_equal(_np(got["labels"]), labels) and np.array_equal(_np(got["info"]), info)
    flat = bank.sample([0, 5, 2], (5, 6, 7), seed=8, mode="random")  # a flat list: one try per slot
    assert _np(flat["info"])[:, :2].tolist() == [[0, 0], [0, 5], [0, 2]]
    # epoch_batches: the plan's candidates and seeds, reproducible, another epoch and another rank differ
    run = lambda **kw: [{k: _np(v) for k, v in b.items()} for b in bank.epoch_batches(2, (5, 6, 7), **kw)]
    a, again, other = run(epoch=0, seed=6, tries=4), run(epoch=0, seed=6, tries=4), run(epoch=1, seed=6, tries=4)
    assert len(a) == 4
    plan = sd.epoch_plan(8, 2, 0, seed=6, tries=4)
    for got, same, (_, cand, s) in zip(a, again, plan):
        want = ref.sample(vols, cand, (5, 6, 7), s, "one_positive")
        assert all(np.array_equal(got[k], w) and np.array_equal(same[k], w) for k, w in zip(("images", "weights", "labels", "info"), want))
    assert any(not np.array_equal(x["images"], y["images"]) for x, y in zip(a, other))
    r0, r1 = run(epoch=0, seed=6, tries=4, rank=0, world=2), run(epoch=0, seed=6, tries=4, rank=1, world=2)
    assert len(r0) == len(r1) == 2
    p0, p1 = sd.epoch_plan(8, 2, 0, seed=6, tries=4, rank=0, world=2), sd.epoch_plan(8, 2, 0, seed=6, tries=4, rank=1, world=2)
    assert all(not np.array_equal(x[1], y[1]) for x, y in zip(p0, p1))  # the two ranks draw different candidate lists
    assert all(not np.array_equal(x["images"], y["images"]) for x, y in zip(r0, r1))
    for i in (0, 5):  # whole(c) round-trips the prepared volume
        image, label, weight = bank.whole(i)
        assert np.array_equal(np.moveaxis(_np(image), 0, -1), vols[i]["image"]) and np.array_equal(_np(label), vols[i]["label"])
        assert np.array_equal(_np(weight), vols[i]["weight"]) and bank.shape(i) == vols[i]["label"].shape


# ---- training and evaluation ---------------------------------------------------------------------------------------------------------------

def _pancreas_bank(shapes, seed):
    rng = np.random.default_rng(seed)
    bank = _sd().PatchBank(1)
    for s in shapes:
        ct = np.clip(rng.normal(0, 150, s), -1024, 1024).astype(np.int16)
        g = np.stack(np.meshgrid(*[np.arange(n) for n in s], indexing="ij"), -1)
        blob = (((g - np.array(s) / 2.0) / (np.array(s) / 4.0)) ** 2).sum(-1) < 1.0
        ct[blob] += 200
        bank.add_pancreas(ct, blob.astype(np.uint8))
    return bank


def test_train_saliency_equals_the_steps_written_out_by_hand():
    """Two steps at patch (16, 16, 16), B = 2, C = 1 on three small Pancreas-form volumes: the same seeds and kernels, so bit for bit."""
    from point_unet_amd import saliency
    sd = _sd()
    bank = _pancreas_bank(((20, 24, 18), (16, 16, 16), (18, 20, 22)), seed=9)
    params = saliency.init_params(1, 2, seed=5)
    P = (16, 16, 16)
    net = saliency.TrainableSaliencyNet(params, 1)
    losses = sd.train_saliency(net, bank, 2, P, batch_size=2, lr=0.01, seed=3)
    assert isinstance(losses, torch.Tensor) and losses.is_cuda and tuple(losses.shape) == (2,) and not losses.requires_grad
    hand = saliency.TrainableSaliencyNet(params, 1)
    opt = saliency.reference_optimizer(hand, lr=0.01)
    by_hand = []
    for epoch in (0, 1):  # three volumes, batches of two: one batch per epoch
        (_, cand, s), = sd.epoch_plan(3, 2, epoch, seed=3, tries=8)
        batch = bank.sample(cand, P, s, "one_positive")
        assert int(batch["info"][:, 5].sum()) > 0  # one_positive: the batch sees the blob
        opt.zero_grad(set_to_none=True)
        loss = hand.loss(batch["images"], batch["labels"], batch["weights"])
        loss.backward()
        opt.step()
        by_hand.append(loss.detach())
    got, want = _np(losses), _np(torch.stack(by_hand))
    print("losses", got, want)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.isfinite(got).all() and 0 < got.min() and got.max() <= 1
    # Every parameter moved -- every one whose gradient is not zero by the network's structure.  Two kinds cannot move, and the test asks of
    # them what the structure says instead (10 of the 158 parameter tensors stay, 29 biases stay within noise):
    #   the bias of a convolution in front of an instance norm: the norm subtracts the channel's mean, so the loss does not depend on the
    #   bias; its gradient is a sum of rounding errors and it carries no weight decay -- it stays within that noise;
    #   the layers at 1/16 resolution: at patch (16, 16, 16) they see a 1 x 1 x 1 volume.  An instance norm over ONE voxel has x - mean = 0,
    #   its output is ReLU(beta) whatever its input and its gamma: the gammas of stride2conv3, down4_conv_* and C5_cfe_* have gradient
    #   exactly 0, and since every path from stride2conv3 / down4_conv_* to the loss runs through a C5_cfe_* norm, which forgets its input,
    #   so have their betas.  They carry no weight decay: they stay bit for bit.  (C5_cfe_*'s betas do reach the loss, and move.)
    normed = {saliency.SCOPE + name + "/bias" for name, _, bias, norm in saliency.layer_table(1, 2) if bias and norm}
    one_voxel = {saliency.SCOPE + name + "/ins_norm/gamma" for name in ("stride2conv3", "down4_conv_0", "down4_conv_1", "C5_cfe_cfe0", "C5_cfe_cfe1_dilation",
                                                                          "C5_cfe_cfe2_dilation", "C5_cfe_cfe3_dilation")}
    one_voxel |= {saliency.SCOPE + name + "/ins_norm/beta" for name in ("stride2conv3", "down4_conv_0", "down4_conv_1")}
    before = saliency.unflatten_params(saliency.flatten_params(params, 1), 1)
    assert one_voxel <= set(before) and normed <= set(before)
    noise, unmoved = [], []
    for (name, p), (name2, q) in zip(net.named_parameters(), hand.named_parameters()):
        assert name == name2 and torch.equal(p, q), name
        change = float(np.abs(_np(p).astype(np.float64) - before[name]).max())
        if name in normed:
            noise.append(change)
        elif name in one_voxel:
            assert change == 0, (name, change)
        elif not change > 0:
            unmoved.append(name)
    print("%d biases in front of an instance norm, largest change %.3e; unmoved: %s" % (len(noise), max(noise), unmoved))
    assert not unmoved, unmoved
    assert len(noise) == len(normed) > 0 and max(noise) <= 1e-5  # (lr 0.01 times 2.9 gradients of rounding noise)


def test_evaluate_saliency_is_binary_dice3d_of_the_argmax():
    from point_unet_amd import saliency
    bank = _pancreas_bank(((16, 32, 16),), seed=12)
    net = saliency.SaliencyNet(saliency.init_params(1, 2, seed=6), 1)
    patch, steps = (16, 16, 16), (16, 8, 16)
    dice, = _sd().evaluate_saliency(bank, net, [0], patch, steps)
    image, label, _ = bank.whole(0)
    pred = np.argmax(_np(saliency.saliency_map(image, net, patch, steps)), axis=-1)
    g = _np(label).astype(np.int64)
    s0, s1, s2 = np.multiply(pred, g).sum(), pred.sum(), g.sum()
    want = (2.0 * s0 + 1e-10) / (s1 + s2 + 1e-10)
    print("dice", dice, want, "predicted", int(s1), "labelled", int(s2))
    assert isinstance(dice, float) and abs(dice - want) <= 1e-12 and s2 > 0
