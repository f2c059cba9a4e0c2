"""include/pointseg_saliency_view.h on the device: ps_patch_sample_view / ps_patch_sample_mixup_view byte-equal to the numpy restatement
(saliency_view_ref.py) between guard bands, in every view, mode and branch of the choice of try; the defining identity on the device (a
second bank of permuted contiguous copies, torch.flip); the axial, unflipped call against the old entries; the flip; reproducibility and
argument errors; train_saliency(direction=, flip=) in both engines and the {view: net} evaluate_saliency fuses."""
import ctypes

import numpy as np
import pytest

import saliency_data_ref as dref
import saliency_view_ref as vref
import test_gpu_saliency_data as tdata
import test_gpu_saliency_mixup as tmix

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

# the volumes where the kernels can go wrong: odd extents (source rows start at any byte), one voxel, one smaller than every patch below on
# every axis of every view
SHAPES = ((7, 41, 37), (9, 20, 23), (1, 1, 1), (3, 2, 4))
GAMMAS = tmix.GAMMAS
PERM = {"axial": (0, 1, 2), "sagittal": (2, 0, 1), "coronal": (1, 0, 2)}


def _sd():
    from point_unet_amd import saliency_data
    return saliency_data


def _np(t):
    return t.detach().cpu().numpy()


def _direct(bank, cand, P, seed, mode, view, flip=None, K=None, gamma=None, shift=0, bad=None):
    """ps_patch_sample_view (K is None) or ps_patch_sample_mixup_view itself, every output `shift` bytes past a 256-byte boundary between
    guard bands.  Returns (rc, outputs as numpy, True when every band is intact, the raw output bytes)."""
    from point_unet_amd import _lib, runtime
    cand = np.ascontiguousarray(cand, dtype=np.int32)
    mixed = K is not None
    B, T = cand.shape[0] - (1 if mixed else 0), cand.shape[1]
    C, P = bank.channels, tuple(P)
    shapes = {"images": ((B,) + P + (C,), np.float32), "weights": ((B,) + P, np.float32),
              "labels": ((B,) + P + (K,), np.float32) if mixed else ((B,) + P, np.int32), "info": ((cand.shape[0], 8), np.int32)}
    bufs = {k: tdata._banded(4 * int(np.prod(s)), shift) for k, (s, _) in shapes.items()}
    images, labels, weights, dims, n = bank.c_tables()
    bank.ctx.use_torch_stream()
    a = dict(ctx=bank.ctx.handle, images=images, labels=labels, weights=weights, dims=dims, n=n, C=C, cand=cand.ctypes.data_as(_lib.c_i32p), B=B, T=T,
             P=(ctypes.c_int64 * 3)(*P), seed=seed, mode=tdata.MODE_ID[mode])
    if mixed:
        g = np.ascontiguousarray(gamma, np.float64)
        a.update(K=K, gamma=g.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    a.update(view=vref.VIEW_ID[view], flip=None if flip is None else (ctypes.c_int32 * len(flip))(*[int(f) for f in flip]),
             oi=runtime.ptr(bufs["images"][1]), ow=runtime.ptr(bufs["weights"][1]), ol=runtime.ptr(bufs["labels"][1]), oinfo=runtime.ptr(bufs["info"][1]))
    a.update(bad or {})
    fn = _lib.lib().ps_patch_sample_mixup_view if mixed else _lib.lib().ps_patch_sample_view
    rc = fn(*a.values())
    torch.cuda.synchronize()
    band = tdata.BAND
    intact = all(bool((full[:band + shift] == 0xA5).all()) and bool((full[band + shift + part.numel():] == 0xA5).all()) for full, part in bufs.values())
    raw = {k: _np(part).copy() for k, (_, part) in bufs.items()}
    return rc, {k: raw[k].view(dt).reshape(s) for k, (s, dt) in shapes.items()}, intact, raw


def _equal_to_the_rule(vols, permuted, bank, cand, P, seed, mode, view, flip, K=None, gamma=None, shift=0):
    from point_unet_amd import _lib
    rc, got, intact, raw = _direct(bank, cand, P, seed, mode, view, flip, K, gamma, shift)
    assert rc == 0, _lib.lib().ps_last_error()
    if K is None:
        images, weights, labels, info = vref.sample_view(vols, cand, P, seed, mode, view, flip, permuted)
    else:
        images, weights, labels, info = vref.sample_mixup_view(vols, cand, P, seed, mode, K, gamma, view, flip, permuted)
    assert np.array_equal(got["info"], info), (got["info"], info)
    assert np.array_equal(got["weights"].view(np.uint32), weights.view(np.uint32))
    assert np.array_equal(got["labels"].view(np.uint32), labels.view(np.uint32))
    assert np.array_equal(got["images"].view(np.uint32), images.view(np.uint32))
    assert intact, "a guard band was written"
    return info, raw


# (C, view patch).  C = 1, 3, 4: TW = 32; C = 16: TW = 8.  (5, 6, 7): P2 * C % 4 != 0 at C = 1, == 0 at C = 4 and 16; (36, 5, 40): more than
# one tile along both tile axes of the sagittal gather, the last ones partial, P2 * C % 4 == 0 with quads that cross voxels at C = 3;
# (16, 16, 16) and (8, 8, 8): P2 % 4 == 0, the 16-byte label and weight rows.
CASES = [(1, (5, 6, 7)), (4, (5, 6, 7)), (16, (5, 6, 7)), (1, (36, 5, 40)), (3, (36, 5, 40)), (16, (36, 5, 40)), (1, (16, 16, 16)), (4, (16, 16, 16)),
         (3, (8, 8, 8)), (4, (8, 8, 8))]
FLIPS = (None, (1, 1, 1, 1), (1, 0, 1, 0), (0, 1, 1, 0), (0, 0, 0, 1))


@pytest.mark.parametrize("view", vref.VIEWS)
@pytest.mark.parametrize("C, P", CASES, ids=["C%d-P%s" % (c, "x".join(map(str, p))) for c, p in CASES])
def test_view_samplers_equal_the_rule_bit_for_bit(C, P, view):
    """Hard and mixed, the three modes, every branch of the choice of try (a slot with ok = 0 among them), every flip pattern; then outputs
    4 bytes past a 16-byte boundary, which take the narrower stores: the same bytes."""
    vols, bank = tdata._make_bank(C, SHAPES, seed=500 + C + P[0])
    permuted = vref.view_bank(vols, view)
    n = len(SHAPES)
    seen, call = {}, 0
    for B, T in ((1, 1), (3, 4)):
        hard, mixed, seed = tdata._cands(n, B, T), tmix._cands(n, B, T), 7 + 13 * B + T
        for mode in dref.MODES:
            for name in ("mixed", "none", "late", "late_all", "first", "forced"):
                if T == 1 and name not in ("mixed", "none"):
                    continue
                flip = FLIPS[call % len(FLIPS)]
                call += 1
                if name != "forced":
                    info, _ = _equal_to_the_rule(vols, permuted, bank, hard[name], P, seed, mode, view, None if flip is None else flip[:B])
                    seen[("hard", mode, name, B, T)] = (tuple(info[:, 0]), tuple(info[:, 6]))
                K = 2 + call % 3  # 2, 3, 4: labels go up to 3, so K = 2 and 3 see labels >= K
                gamma = [GAMMAS[(call + b) % len(GAMMAS)] for b in range(B)]
                info, _ = _equal_to_the_rule(vols, permuted, bank, mixed[name], P, seed, mode, view, None if flip is None else flip[:B + 1], K, gamma)
                seen[("mixed", mode, name, B, T)] = (tuple(info[:, 0]), tuple(info[:, 6]))
    # each branch of the choice was taken, in the view's own boxes
    assert seen[("hard", "one_positive", "none", 3, 4)] == ((0, 0, 3), (1, 1, 0)) and seen[("hard", "all_positive", "none", 3, 4)] == ((3, 3, 3), (0, 0, 0))
    assert seen[("hard", "one_positive", "late", 3, 4)] == ((0, 0, 3), (1, 1, 1)) and seen[("hard", "all_positive", "late_all", 3, 4)] == ((3, 3, 3), (1, 1, 1))
    assert seen[("hard", "one_positive", "first", 3, 4)] == ((0, 0, 0), (1, 1, 1)) and seen[("hard", "random", "none", 3, 4)] == ((0, 0, 0), (1, 1, 1))
    assert seen[("hard", "one_positive", "none", 1, 1)] == ((0,), (0,))
    assert seen[("mixed", "one_positive", "forced", 3, 4)] == ((0, 0, 3, 0), (1, 1, 1, 1)) and seen[("mixed", "one_positive", "none", 3, 4)] == ((0, 0, 3, 0), (1, 1, 0, 1))
    assert seen[("mixed", "all_positive", "none", 3, 4)] == ((3, 3, 3, 3), (0, 0, 0, 0)) and seen[("mixed", "one_positive", "first", 3, 4)] == ((0, 0, 0, 0), (1, 1, 1, 1))
    # another alignment of the outputs, the same bytes
    hard, mixed = tdata._cands(n, 3, 4)["mixed"], tmix._cands(n, 3, 4)["mixed"]
    gamma = [GAMMAS[3], GAMMAS[2], GAMMAS[4]]
    for flip in (None, (1, 0, 1, 1)):
        _, raw = _equal_to_the_rule(vols, permuted, bank, hard, P, 5, "one_positive", view, None if flip is None else flip[:3])
        _, shifted = _equal_to_the_rule(vols, permuted, bank, hard, P, 5, "one_positive", view, None if flip is None else flip[:3], shift=4)
        assert all(np.array_equal(raw[k], shifted[k]) for k in raw)
        _, raw = _equal_to_the_rule(vols, permuted, bank, mixed, P, 5, "one_positive", view, flip, 4, gamma)
        _, shifted = _equal_to_the_rule(vols, permuted, bank, mixed, P, 5, "one_positive", view, flip, 4, gamma, shift=4)
        assert all(np.array_equal(raw[k], shifted[k]) for k in raw)


# ---- the defining identity, on the device -------------------------------------------------------------------------------------------------------

def _permuted_bank(vols, C, view):
    """A second PatchBank of permute(...).contiguous() copies: the route the view entries replace."""
    bank = _sd().PatchBank(C)
    ax = PERM[view]
    for v in vols:
        image, label, weight = (torch.from_numpy(v[k]).cuda() for k in ("image", "label", "weight"))
        bank.add_prepared(image.permute(*ax, 3).contiguous(), label.permute(*ax).contiguous(), weight.permute(*ax).contiguous())
    return bank


def _flip_flagged(t, bits):
    out = t.clone()
    for b, f in enumerate(bits):
        if f:
            out[b] = torch.flip(t[b], (2,))
    return out


@pytest.mark.parametrize("view", ["sagittal", "coronal"])
@pytest.mark.parametrize("C, P", [(1, (5, 6, 7)), (4, (16, 16, 16)), (3, (36, 5, 40))], ids=["C1-P5", "C4-P16", "C3-P36"])
def test_view_samplers_equal_the_old_samplers_on_permuted_copies(C, P, view):
    vols, bank = tdata._make_bank(C, SHAPES, seed=61)
    copies = _permuted_bank(vols, C, view)
    n, K = len(SHAPES), 4
    bits = [1, 0, 1, 1]
    for mode, name in (("one_positive", "mixed"), ("all_positive", "late_all"), ("one_positive", "none"), ("random", "mixed")):
        cand = tdata._cands(n, 4, 4)[name]
        got, want = bank.sample(cand, P, 21, mode, direction=view, flip=bits), copies.sample(cand, P, 21, mode)
        for k in ("images", "weights", "labels"):
            assert torch.equal(got[k].view(torch.int32), _flip_flagged(want[k], bits).view(torch.int32)), (mode, name, k)
        assert torch.equal(got["info"][:, :7], want["info"][:, :7]) and got["info"][:, 7].tolist() == bits
        # mixed, unflipped: the old mixed sampler on the copies
        mcand = tmix._cands(n, 3, 4)[name]
        gamma = np.array([GAMMAS[3], GAMMAS[2], GAMMAS[4]])
        got, want = bank.sample(mcand, P, 21, mode, mixup=K, gamma=gamma, direction=view), copies.sample(mcand, P, 21, mode, mixup=K, gamma=gamma)
        assert all(torch.equal(got[k].view(torch.int32), want[k].view(torch.int32)) for k in ("images", "weights", "labels", "info"))
        if mode == "one_positive":
            continue
        # mixed, flipped: for the modes whose choice does not single out a sample the mixed batch is the plain one at B + 1 slots on the
        # copies, its flagged samples flipped, mixed by eager torch ops (two products and a sum, each its own kernel)
        got, plain = bank.sample(mcand, P, 21, mode, mixup=K, gamma=gamma, direction=view, flip=bits), copies.sample(mcand, P, 21, mode)
        g, h = torch.from_numpy(gamma.astype(np.float32)).cuda(), torch.from_numpy((1.0 - gamma).astype(np.float32)).cuda()

        def mix(t):
            shape = (3,) + (1,) * (t.dim() - 1)
            a, b = g.reshape(shape) * t[:-1], h.reshape(shape) * t[1:]
            return a + b

        image, weight, label = (_flip_flagged(plain[k], bits) for k in ("images", "weights", "labels"))
        hot = torch.nn.functional.one_hot(label.long(), K).to(torch.float32)
        assert torch.equal(got["images"], mix(image)) and torch.equal(got["labels"], mix(hot))
        assert torch.equal(got["weights"], ((weight[:-1] != 0) | (weight[1:] != 0)).to(torch.float32))
        assert torch.equal(got["info"][:, :7], plain["info"][:, :7]) and got["info"][:, 7].tolist() == bits


# ---- pass-through -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C, P", [(1, (5, 6, 7)), (4, (16, 16, 16))], ids=["C1-P5", "C4-P16"])
def test_axial_unflipped_is_the_old_entries(C, P):
    """direction="axial", flip=None through the new entries gives the bytes ps_patch_sample / ps_patch_sample_mixup give, called directly."""
    vols, bank = tdata._make_bank(C, SHAPES, seed=71)
    n = len(SHAPES)
    for mode, name in (("one_positive", "mixed"), ("all_positive", "late_all"), ("one_positive", "none")):
        cand = tdata._cands(n, 3, 4)[name]
        rc, old, intact, _ = tdata._direct(bank, cand, P, 9, mode)
        assert rc == 0 and intact and int(old["info"][:, 7].max()) == 0
        new = bank.sample(cand, P, 9, mode, direction="axial", flip=None)
        assert all(np.array_equal(_np(new[k]).view(np.uint32), old[k].view(np.uint32)) for k in ("images", "weights", "labels", "info"))
        rc, view0, intact, _ = _direct(bank, cand, P, 9, mode, "axial", [0, 0, 0])  # all-zero bits are no flip
        assert rc == 0 and intact and all(np.array_equal(view0[k].view(np.uint32), old[k].view(np.uint32)) for k in old)
        mcand, gamma = tmix._cands(n, 3, 4)[name], [GAMMAS[3], GAMMAS[2], GAMMAS[4]]
        old, _ = tmix._direct(bank, mcand, P, 9, mode, 3, gamma)
        new = bank.sample(mcand, P, 9, mode, mixup=3, gamma=gamma)
        for k, k_old in (("images", "images"), ("weights", "weights"), ("labels", "soft"), ("info", "info")):
            assert np.array_equal(_np(new[k]).view(np.uint32), old[k_old].view(np.uint32)), k


# ---- flip -----------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("view", vref.VIEWS)
def test_flip_is_torch_flip_of_the_last_view_axis(view):
    for C, P in ((1, (5, 6, 7)), (3, (8, 8, 8)), (4, (36, 5, 40))):
        vols, bank = tdata._make_bank(C, SHAPES, seed=81)
        cand = tdata._cands(len(SHAPES), 3, 4)["mixed"]
        plain = bank.sample(cand, P, 13, "one_positive", direction=view)
        flipped = bank.sample(cand, P, 13, "one_positive", direction=view, flip=[1, 1, 1])
        for k in ("images", "weights", "labels"):  # the fill is mirrored with the image
            assert torch.equal(flipped[k].view(torch.int32), torch.flip(plain[k], (3,)).view(torch.int32)), k
            assert not torch.equal(flipped[k], plain[k])
        assert torch.equal(flipped["info"][:, :7], plain["info"][:, :7]) and flipped["info"][:, 7].tolist() == [1, 1, 1] and plain["info"][:, 7].tolist() == [0] * 3
        # mixed: a flip on drawn sample b + 1 shows in slots b and b + 1, nowhere else
        mcand, gamma = np.array([[0, 1], [1, 0], [0, 1], [1, 0]]), [0.25, 0.5, 0.75]  # (the two large labelled volumes: no patch is its own mirror)
        base = bank.sample(mcand, P, 13, "random", mixup=4, gamma=gamma, direction=view)
        one = bank.sample(mcand, P, 13, "random", mixup=4, gamma=gamma, direction=view, flip=[0, 0, 1, 0])
        assert [not torch.equal(base["images"][b], one["images"][b]) for b in range(3)] == [False, True, True]
        assert [not torch.equal(base["labels"][b], one["labels"][b]) for b in range(3)] == [False, True, True]
        assert one["info"][:, 7].tolist() == [0, 0, 1, 0] and torch.equal(one["info"][:, :7], base["info"][:, :7])
        # all four drawn samples flipped: mixing commutes with the mirror
        every = bank.sample(mcand, P, 13, "random", mixup=4, gamma=gamma, direction=view, flip=[1, 1, 1, 1])
        assert all(torch.equal(every[k].view(torch.int32), torch.flip(base[k], (3,)).view(torch.int32)) for k in ("images", "weights", "labels"))
    # flip="random": the bits of numpy's default generator at the batch's seed, whatever gamma's draw
    drawn = bank.sample(mcand, P, 13, "random", mixup=4, direction=view, flip="random")
    bits = np.random.default_rng(13).integers(0, 2, 4).tolist()
    assert drawn["info"][:, 7].tolist() == bits and np.array_equal(drawn["gamma"], np.random.default_rng(13).beta(0.4, 0.4, 3))
    again = bank.sample(mcand, P, 13, "random", mixup=4, gamma=drawn["gamma"], direction=view, flip=bits)
    assert all(torch.equal(drawn[k], again[k]) for k in ("images", "weights", "labels", "info"))


# ---- reproducibility and errors ----------------------------------------------------------------------------------------------------------------

def test_view_samplers_are_deterministic_across_calls_contexts_and_streams():
    from point_unet_amd import runtime
    shapes = ((9, 20, 23), (17, 33, 19))
    vols, bank = tdata._make_bank(4, shapes, seed=1)
    _, bank2 = tdata._make_bank(4, shapes, seed=1, ctx=runtime.default_context(0))
    hard, mixed = tdata._cands(2, 3, 4)["mixed"], tmix._cands(2, 3, 4)["mixed"]
    torch.cuda.synchronize()
    for view in ("sagittal", "coronal"):
        for kw, cand in ((dict(flip=[1, 0, 1]), hard), (dict(flip=[1, 0, 1, 1], mixup=3, gamma=[0.3, 0.6, 0.9]), mixed)):
            draw = lambda b, seed=21: b.sample(cand, (5, 6, 7), seed=seed, direction=view, **kw)
            first, again, other = draw(bank), draw(bank), draw(bank2)
            side = torch.cuda.Stream()
            with torch.cuda.stream(side):
                private = draw(bank)
            torch.cuda.synchronize()
            for k in ("images", "weights", "labels", "info"):
                for o in (again, other, private):
                    assert torch.equal(first[k].view(torch.int32), o[k].view(torch.int32)), (view, k)
            assert not torch.equal(first["info"], draw(bank, 22)["info"])


def test_view_argument_errors_leave_the_outputs_untouched():
    from point_unet_amd import _lib
    vols, bank = tdata._make_bank(1, ((9, 20, 23),), seed=2)
    err = _lib.lib().ps_last_error
    i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)
    for K, cand in ((None, np.array([[0, 1], [1, 0]])), (2, np.array([[0, 1], [1, 0], [0, 0]]))):
        gamma = None if K is None else [0.25, 0.5]
        for kw, word in ((dict(view=3), b"view = 3"), (dict(view=-1), b"view = -1"), (dict(flip=i32(0, 2, 0)), b"flip[1] = 2"), (dict(flip=i32(-1, 0, 0)), b"flip[0] = -1"),
                         (dict(B=65), b"B = 65"), (dict(T=0), b"T = 0"), (dict(C=17), b"C = 17"), (dict(mode=5), b"mode = 5"), (dict(n=1), b"cand[0, 1] = 1"),
                         (dict(P=(ctypes.c_int64 * 3)(5, 0, 7)), b"P = [5, 0, 7]"), (dict(ow=None), b"NULL out_images"), (dict(images=None), b"NULL images"),
                         (dict(dims=(ctypes.c_int64 * 6)(9, 20, 23, 9, 20, 0)), b"dims of volume 1"), (dict(P=(ctypes.c_int64 * 3)(1, 1 << 23, 1)), b"sagittal")):
            rc, _, intact, raw = _direct(bank, cand, (5, 6, 7), 3, "one_positive", "sagittal", None, K, gamma, bad=kw)
            assert rc == 1 and word in err(), (kw, err())
            assert intact and all(bool((v == 0xA5).all()) for v in raw.values()), kw
        rc, _, intact, _ = _direct(bank, cand, (5, 6, 7), 3, "one_positive", "sagittal", [1, 0] if K is None else [1, 0, 1], K, gamma)
        assert rc == 0 and intact


# ---- the Python surface -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("engine", ["autograd", "native"])
def test_train_saliency_in_a_view_equals_the_steps_written_out_by_hand(engine):
    """Two steps at view patch (16, 16, 16), B = 2, direction="sagittal", flip="random" on three small Pancreas-form volumes: the same seeds and
    kernels, so bit for bit."""
    from point_unet_amd import saliency as sal
    sd = _sd()
    bank = tdata._pancreas_bank(((20, 24, 18), (16, 16, 16), (18, 20, 22)), seed=9)
    params = sal.init_params(1, 2, seed=5)
    P = (16, 16, 16)
    make = (lambda: sal.SaliencyTrainer(params, 1, 2)) if engine == "native" else (lambda: sal.TrainableSaliencyNet(params, 1))
    net, hand = make(), make()
    losses = sd.train_saliency(net, bank, 2, P, batch_size=2, lr=0.01, seed=3, engine=engine, direction="sagittal", flip="random")
    opt = None if engine == "native" else sal.reference_optimizer(hand, lr=0.01)
    by_hand, bits = [], []
    for epoch in (0, 1):  # three volumes, batches of two: one batch per epoch
        (_, cand, s), = sd.epoch_plan(3, 2, epoch, seed=3, tries=8)
        flip = np.random.default_rng(s & 0xFFFFFFFF).integers(0, 2, 2).tolist()
        batch = bank.sample(cand, P, s, "one_positive", direction="sagittal", flip=flip)
        plain = bank.sample(cand, P, s, "one_positive", direction="sagittal")
        assert batch["info"][:, 7].tolist() == flip and torch.equal(batch["images"], _flip_flagged(plain["images"], flip))
        bits += flip
        if engine == "native":
            by_hand.append(hand.step(batch["images"], batch["labels"], batch["weights"], 0.01).clone())
        else:
            opt.zero_grad(set_to_none=True)
            loss = hand.loss(batch["images"], batch["labels"], batch["weights"])
            loss.backward()
            opt.step()
            by_hand.append(loss.detach())
    got, want = _np(losses), _np(torch.stack(by_hand))
    print("losses", got, want, "flip bits", bits)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and np.isfinite(got).all()
    if engine == "native":
        assert torch.equal(hand.flat, net.flat) and torch.equal(hand.accum, net.accum)
    else:
        assert all(torch.equal(p, q) for p, q in zip(net.parameters(), hand.parameters()))
    # the view matters: the axial run of the same steps sees other patches
    axial = sd.train_saliency(make(), bank, 1, P, batch_size=2, lr=0.01, seed=3, engine=engine)
    assert not torch.equal(axial[0], losses[0])


def test_three_views_trained_from_one_bank_are_fused_by_evaluate_saliency():
    """Two steps per view on ONE three-volume bank give the {view: net} that evaluate_saliency fuses."""
    from point_unet_amd import saliency as sal
    sd = _sd()
    bank = tdata._pancreas_bank(((20, 24, 18), (16, 32, 16), (18, 20, 22)), seed=12)
    P = (16, 16, 16)
    nets = {}
    for k, view in enumerate(vref.VIEWS):
        nets[view] = sal.TrainableSaliencyNet(sal.init_params(1, 2, seed=6 + k), 1)
        losses = sd.train_saliency(nets[view], bank, 2, P, batch_size=2, lr=0.01, seed=3, direction=view, flip="random")
        assert tuple(losses.shape) == (2,) and bool(torch.isfinite(losses).all())
    dice = sd.evaluate_saliency(bank, nets, range(3), P, (16, 8, 16))
    print("dice", dice)
    assert len(dice) == 3 and all(isinstance(d, float) and np.isfinite(d) and 0.0 <= d <= 1.0 for d in dice)
