"""The saliency network's data on the device (include/pointseg_saliency_data.h, csrc/saliency_data.hip): what the reference does per
sample on the host -- crop_brain_region / load_pancreas_img (SaliencyAttention/utils.py:30-78), sampler3d and BatchData's reject loop
(SaliencyAttention/data_sampler.py:77-88, 169-214) behind MultiProcessMapDataZMQ workers -- as volumes prepared once and kept in HBM, and
batches of patches drawn there by a stated rule with no host read.  PatchBank is to TrainableSaliencyNet what dataset.CloudBank is to the
point network's Trainer; train_saliency is the loop of train.py:83-110 over it, evaluate_saliency the Dice of EvalCallback / eval_pancreas.

config.MIXUP (include/pointseg_saliency_mixup.h): PatchBank.sample(mixup=num_classes) draws B + 1 samples and mixes neighbour pairs on the
device into images, or-ed weights and soft labels, which the loss and both training engines take.  config.DIRECTION and sampler3d's
np.flip(..., -1) (include/pointseg_saliency_view.h): sample(direction=, flip=) draws the batch through an anatomical view of the SAME
resident volumes, with no permuted or mirrored copy, so one bank trains the three networks saliency_map fuses:

    nets = {}
    for view in ("axial", "sagittal", "coronal"):           # P is in the view's axes
        nets[view] = TrainableSaliencyNet(init_params(1, 2, seed=0), 1)
        train_saliency(nets[view], bank, steps=250, patch=P, direction=view, flip="random")
    dice = evaluate_saliency(bank, nets, range(len(bank)), P, steps)    # {view: net}: fused as MULTI_VIEW fuses them

The training step behind one call is saliency.SaliencyTrainer (train_saliency's engine="native");
data-parallel training: hook built, checked with an in-process callback; no multi-process run made."""
import ctypes

import numpy as np
import torch

from . import _lib, runtime
from .dataset import _hash32, batch_seed

MODES = {"random": _lib.PS_PATCH_RANDOM, "all_positive": _lib.PS_PATCH_ALL_POSITIVE, "one_positive": _lib.PS_PATCH_ONE_POSITIVE}
_M32 = 0xFFFFFFFF
_INDEX_MUL = 2654435761


def shuffled_ids(n, s):
    """The volume ids 0 .. n-1 in ascending order of hash32(i * 2654435761 ^ s) (ties by id): the hashed shuffle of the samplers."""
    keys = [(_hash32(((i * _INDEX_MUL) & _M32) ^ s), i) for i in range(int(n))]
    return [i for _, i in sorted(keys)]


def epoch_plan(n_volumes, batch_size, epoch, seed=0, tries=8, rank=0, world=1):
    """[(batch index, cand int32 [batch_size, tries], seed)] of one epoch on one rank.  The reference shuffles the list of volumes
    (DataFromList(shuffle=True)), takes one patch per datapoint and lets BatchData skip a datapoint it rejects for the next of the list.
    Here the list is a stream of hashed shuffles -- pass p is shuffled_ids(n, hash32(hash32(seed + 0x9E3779B9 (epoch + 1)) + 0x85EBCA6B (p + 1))),
    position q of the stream is entry q % n of pass q // n -- and batch j owns positions j * (batch_size + tries - 1) onwards:
    cand[b, t] is position b + t of them, so a slot's next try is the next datapoint.  An epoch has n // batch_size batches over all ranks;
    rank r of `world` takes batches r, r + world, ..., each with dataset.batch_seed(seed, epoch, j, rank)."""
    n, bs, T, world, rank = int(n_volumes), int(batch_size), int(tries), int(world), int(rank)
    if n < 1 or bs < 1 or T < 1 or world < 1 or not 0 <= rank < world:
        raise ValueError("epoch_plan: need n_volumes, batch_size, tries >= 1 and 0 <= rank < world")
    s_epoch = _hash32(int(seed) + 0x9E3779B9 * (int(epoch) + 1))
    passes = {}

    def at(q):
        p = q // n
        if p not in passes:
            passes[p] = shuffled_ids(n, _hash32(s_epoch + 0x85EBCA6B * (p + 1)))
        return passes[p][q % n]

    span = bs + T - 1
    plan = []
    for j in range(rank, n // bs, world):
        cand = np.array([[at(j * span + b + t) for t in range(T)] for b in range(bs)], dtype=np.int32)
        plan.append((j, cand, batch_seed(int(seed), int(epoch), j, rank)))
    return plan


class PatchBank:
    """Prepared volumes resident on one GPU -- image f32 [d, h, w, C] (channels-last: a patch row is one contiguous run), label u8
    [d, h, w], weight u8 [d, h, w] -- and training batches drawn from them on the device (ps_patch_sample).

        bank = PatchBank(channels=1)
        for ct, label in cases:                       # the caller reads the files
            bank.add_pancreas(ct, label)
        losses = train_saliency(net, bank, steps=250, patch=(64, 160, 160))
        dice = evaluate_saliency(bank, net, range(len(bank)), (64, 160, 160), (48, 118, 118))

    Every call runs on torch's current stream; consecutive draws on different streams are ordered through an event (they share the
    context's workspace).  Adding a volume synchronises once in the BraTS form (the crop's box comes to the host), never in the Pancreas
    form; sample() never does."""

    def __init__(self, channels, device=0, ctx=None):
        self.channels = int(channels)
        if not 1 <= self.channels <= _lib.PS_PATCH_MAX_C:
            raise ValueError("PatchBank: channels must be in [1, %d]" % _lib.PS_PATCH_MAX_C)
        self.device = torch.device("cuda", int(device))
        self._ctx = ctx      # (its own context otherwise, created with the first volume: arguments are checked before the GPU is touched)
        self._vols = []      # (image, label, weight, (bbmin, bbmax))
        self._tables = None  # the ctypes tables of ps_patch_sample, rebuilt after a volume was added
        self._done = None

    def __len__(self):
        return len(self._vols)

    @property
    def ctx(self):
        if self._ctx is None:
            self._ctx = runtime.Context(self.device.index)
        return self._ctx

    def shape(self, c):
        """(d, h, w) of prepared volume c."""
        return tuple(self._vols[c][1].shape)

    def bbox(self, c):
        """(bbmin, bbmax), inclusive, of volume c inside the array it was prepared from (crop_brain_region's fifth result; the whole array
        in the Pancreas form)."""
        return self._vols[c][3]

    def whole(self, c):
        """(image f32 [C, d, h, w], label u8 [d, h, w], weight u8 [d, h, w]) of volume c, CUDA tensors: what sampler3d_whole is handed
        (data_sampler.py:216-244), the image ready for saliency.saliency_map."""
        image, label, weight, _ = self._vols[c]
        return image.permute(3, 0, 1, 2).contiguous(), label, weight

    def _dev(self, a, who, name, dtype=None):
        if isinstance(a, torch.Tensor):
            if not a.is_cuda:
                raise ValueError("%s: %s must be a numpy array or a CUDA tensor, got a CPU tensor" % (who, name))
            t = a
        else:
            t = torch.from_numpy(np.ascontiguousarray(a))
        return t.to(device=self.device, dtype=dtype if dtype is not None else t.dtype).contiguous()

    def _keep(self, image, label, weight, box):
        self._vols.append((image, label, weight, box))
        self._tables = None
        return len(self._vols) - 1

    def add_prepared(self, image, label, weight, bbox=None):
        """A volume that is prepared already (the reference's cached `preprocessed` entry): image [d, h, w, C] float32, label and weight
        [d, h, w] with values 0 .. 255; numpy arrays or CUDA tensors.  Returns the volume's id."""
        who = "PatchBank.add_prepared"
        image = self._dev(image, who, "image", torch.float32)
        label, weight = self._dev(label, who, "label", torch.uint8), self._dev(weight, who, "weight", torch.uint8)
        if image.dim() != 4 or image.shape[3] != self.channels or min(image.shape) < 1:
            raise ValueError("%s: image must be [d, h, w, %d], got %s" % (who, self.channels, tuple(image.shape)))
        if label.shape != image.shape[:3] or weight.shape != image.shape[:3]:
            raise ValueError("%s: label and weight must be [d, h, w] like the image" % who)
        d, h, w = label.shape
        return self._keep(image, label, weight, bbox if bbox is not None else ([0, 0, 0], [d - 1, h - 1, w - 1]))

    def add_brats(self, raw, seg=None, num_class=2, margin=5):
        """crop_brain_region (utils.py:30-60): raw [C, D, H, W] (the modalities in the reference's sorted order), seg [D, H, W] integer or
        None.  The box of raw[0] != 0 grown by `margin`, every modality z-scored over its own voxels > 0 inside it (zeros stay 0), weight =
        raw[0] > 0, labels 4 -> 3 (num_class == 4) or 4, 2 -> 1.  Returns the volume's id.  Raises when raw[0] is all zero or a modality
        cannot be normalised."""
        who = "PatchBank.add_brats"
        raw = self._dev(raw, who, "raw", torch.float32)
        if raw.dim() != 4 or raw.shape[0] != self.channels:
            raise ValueError("%s: raw must be [%d, D, H, W], got %s" % (who, self.channels, tuple(raw.shape)))
        C, D, H, W = raw.shape
        if seg is not None:
            seg = self._dev(seg, who, "seg")
            if seg.dtype.is_floating_point or tuple(seg.shape) != (D, H, W):
                raise ValueError("%s: seg must be an integer [%d, %d, %d] array" % (who, D, H, W))
            seg = seg.to(torch.int32).contiguous()
        self.ctx.use_torch_stream()
        lib = _lib.lib()
        box = (ctypes.c_int64 * 6)()
        stats = (ctypes.c_double * (2 * C))()
        _lib.check(lib.ps_saliency_brats_measure(self.ctx.handle, runtime.ptr(raw), C, D, H, W, int(margin), box, stats))
        d, h, w = (box[3 + a] - box[a] + 1 for a in range(3))
        image = torch.empty((d, h, w, C), dtype=torch.float32, device=self.device)
        label = torch.empty((d, h, w), dtype=torch.uint8, device=self.device)
        weight = torch.empty((d, h, w), dtype=torch.uint8, device=self.device)
        _lib.check(lib.ps_saliency_brats_apply(self.ctx.handle, runtime.ptr(raw), runtime.ptr(seg), C, D, H, W, int(num_class), box, stats, runtime.ptr(image),
                                               runtime.ptr(label), runtime.ptr(weight)))
        return self._keep(image, label, weight, (list(box[:3]), list(box[3:])))

    def add_pancreas(self, ct, label=None):
        """load_pancreas_img (utils.py:62-78): ct [D, H, W] (int16 stays int16, anything else is taken as float32) -> (ct + 100) / 340,
        weight 1, the label unchanged (values 0 .. 255).  No crop.  Returns the volume's id."""
        who = "PatchBank.add_pancreas"
        if self.channels != 1:
            raise ValueError("%s: the Pancreas form has one channel, this bank %d" % (who, self.channels))
        ct = self._dev(ct, who, "ct")
        if ct.dim() != 3:
            raise ValueError("%s: ct must be [D, H, W], got %s" % (who, tuple(ct.shape)))
        if ct.dtype != torch.int16:
            ct = ct.to(torch.float32).contiguous()
        if label is not None:
            label = self._dev(label, who, "label")
            if label.dtype.is_floating_point or label.shape != ct.shape:
                raise ValueError("%s: label must be an integer array of ct's shape" % who)
            label = label.to(torch.uint8).contiguous()
        D, H, W = ct.shape
        image = torch.empty((D, H, W, 1), dtype=torch.float32, device=self.device)
        out_label = torch.empty((D, H, W), dtype=torch.uint8, device=self.device)
        weight = torch.empty((D, H, W), dtype=torch.uint8, device=self.device)
        self.ctx.use_torch_stream()
        dtype = _lib.PS_VOLUME_I16 if ct.dtype == torch.int16 else _lib.PS_VOLUME_F32
        _lib.check(_lib.lib().ps_saliency_pancreas_prepare(self.ctx.handle, runtime.ptr(ct), dtype, ct.numel(), runtime.ptr(label), runtime.ptr(image),
                                                           runtime.ptr(out_label), runtime.ptr(weight)))
        return self._keep(image, out_label, weight, ([0, 0, 0], [D - 1, H - 1, W - 1]))

    def c_tables(self):
        """(images, labels, weights, dims, n): the host tables ps_patch_sample takes."""
        if self._tables is None:
            n = len(self._vols)
            ptrs = [(ctypes.c_void_p * max(n, 1))(*[v[k].data_ptr() for v in self._vols]) for k in range(3)]
            dims = (ctypes.c_int64 * (3 * max(n, 1)))(*[int(e) for v in self._vols for e in v[1].shape])
            self._tables = (ptrs[0], ptrs[1], ptrs[2], dims, n)
        return self._tables

    def _view_args(self, who, direction, flip, drawn, seed):
        """(the PS_VIEW_* value, the flip bits as a ctypes int32 array or None) of sample's direction and flip, for `drawn` samples."""
        if direction not in _lib.SALIENCY_VIEWS:
            raise ValueError("%s: direction must be one of %s, got %r" % (who, sorted(_lib.SALIENCY_VIEWS), direction))
        if flip is None:
            return _lib.SALIENCY_VIEWS[direction], None
        if isinstance(flip, str):
            if flip != "random":
                raise ValueError("%s: flip must be None, 'random' or %d values of 0 / 1, got %r" % (who, drawn, flip))
            bits = np.random.default_rng(int(seed) & _M32).integers(0, 2, drawn)  # (a generator of its own: gamma's draw does not move it)
        else:
            bits = np.asarray(flip)
            if bits.shape != (drawn,) or not np.isin(bits, (0, 1)).all():
                raise ValueError("%s: flip must be None, 'random' or %d values of 0 / 1 (one per drawn sample)" % (who, drawn))
        return _lib.SALIENCY_VIEWS[direction], (ctypes.c_int32 * drawn)(*[int(v) for v in bits])

    def sample(self, cand, patch, seed=0, mode="one_positive", mixup=None, gamma=None, direction="axial", flip=None):
        """One batch, drawn on the device on torch's current stream: cand [B, T] volume ids (cand[b, t] is try t of slot b; a flat [B]
        list is T = 1), patch (P0, P1, P2).  Returns {"images" f32 [B, P0, P1, P2, C], "weights" f32 [B, P0, P1, P2], "labels" i32
        [B, P0, P1, P2], "info" i32 [B, 8] = (try, volume, c0, c1, c2, pos, ok, 0)}, CUDA tensors: the first three are what
        TrainableSaliencyNet.loss takes (info's last column is the sample's flip bit).  info's ok is 0 for a slot none of whose tries met the mode's demand (it holds the last try).

        mixup=K, the class count (config.MIXUP, ps_patch_sample_mixup): cand is [B + 1, T], one row per DRAWN sample, and slot b of the B
        mixed slots is gamma[b] * sample b + (1 - gamma[b]) * sample b + 1.  gamma: B float64 values in [0, 1]; None draws
        np.random.default_rng(seed).beta(0.4, 0.4, B) on the host.  "labels" is then f32 [B, P0, P1, P2, K] (soft labels), "info" is
        [B + 1, 8], one row per drawn sample, and "gamma" (float64 numpy [B]) is returned with them.

        direction (config.DIRECTION; "axial", "sagittal" or "coronal", the names saliency_map takes; ps_patch_sample_view): every candidate
        volume is seen as transpose_volumes shows it -- sagittal view[i, j, k] = vol[j, k, i], coronal view[i, j, k] = vol[j, i, k] -- and
        patch, the centres in info and the outputs are in the VIEW's axes; no permuted copy of a volume is made.  flip: None, a sequence of
        0 / 1 per DRAWN sample (B, or B + 1 with mixup), or "random" (np.random.default_rng(seed).integers(0, 2, drawn) on the host, a
        generator of its own): a flagged sample is mirrored along the view's last axis -- image, fill, weight and label, before mixing --
        and info[:, 7] carries the bits.  The defaults give the bytes of ps_patch_sample / ps_patch_sample_mixup."""
        who = "PatchBank.sample"
        if mode not in MODES:
            raise ValueError("%s: mode must be one of %s" % (who, sorted(MODES)))
        if mixup is None and gamma is not None:
            raise ValueError("%s: gamma is mixup's argument" % who)
        if mixup is not None and (isinstance(mixup, bool) or int(mixup) != mixup or not 2 <= int(mixup) <= 16):
            raise ValueError("%s: mixup must be the class count, an integer in [2, 16], got %r" % (who, mixup))
        cand = np.asarray(cand)
        if cand.ndim == 1:
            cand = cand[:, None]
        if cand.ndim != 2 or cand.size == 0 or cand.dtype.kind not in "iu":
            raise ValueError("%s: cand must be a non-empty integer [B, T] array" % who)
        if len(self) == 0 or cand.min() < 0 or cand.max() >= len(self):
            raise ValueError("%s: volume ids must be in [0, %d)" % (who, len(self)))
        cand = np.ascontiguousarray(cand, dtype=np.int32)
        B, T = cand.shape
        P = tuple(int(p) for p in patch)
        if len(P) != 3 or min(P) < 1:
            raise ValueError("%s: patch must be three extents >= 1, got %s" % (who, (patch,)))
        if mixup is not None:
            return self._sample_mixup(cand, P, seed, mode, int(mixup), gamma, direction, flip)
        view, bits = self._view_args(who, direction, flip, B, seed)
        C, dev = self.channels, self.device
        stream = torch.cuda.current_stream(dev)
        if self._done is not None:
            stream.wait_event(self._done)
        out = {"images": torch.empty((B,) + P + (C,), dtype=torch.float32, device=dev), "weights": torch.empty((B,) + P, dtype=torch.float32, device=dev),
               "labels": torch.empty((B,) + P, dtype=torch.int32, device=dev), "info": torch.empty((B, 8), dtype=torch.int32, device=dev)}
        images, labels, weights, dims, n = self.c_tables()
        self.ctx.use_torch_stream()
        _lib.check(_lib.lib().ps_patch_sample_view(self.ctx.handle, images, labels, weights, dims, n, C, cand.ctypes.data_as(_lib.c_i32p), B, T,
                                                   (ctypes.c_int64 * 3)(*P), int(seed) & _M32, MODES[mode], view, bits, runtime.ptr(out["images"]),
                                                   runtime.ptr(out["weights"]), runtime.ptr(out["labels"]), runtime.ptr(out["info"])))
        self._done = torch.cuda.Event()
        self._done.record(stream)
        return out

    def _sample_mixup(self, cand, P, seed, mode, K, gamma, direction="axial", flip=None):
        who = "PatchBank.sample"
        B, T = cand.shape[0] - 1, cand.shape[1]
        if not 1 <= B <= _lib.PS_PATCH_MAX_B - 1:
            raise ValueError("%s: with mixup cand must be [B + 1, T] with B in [1, %d], got %s" % (who, _lib.PS_PATCH_MAX_B - 1, cand.shape))
        view, bits = self._view_args(who, direction, flip, B + 1, seed)
        if gamma is None:
            gamma = np.random.default_rng(int(seed) & _M32).beta(0.4, 0.4, B)
        gamma = np.ascontiguousarray(gamma, dtype=np.float64)
        if gamma.shape != (B,) or not np.all(np.isfinite(gamma)) or gamma.min() < 0.0 or gamma.max() > 1.0:
            raise ValueError("%s: gamma must be %d finite values in [0, 1]" % (who, B))
        C, dev = self.channels, self.device
        stream = torch.cuda.current_stream(dev)
        if self._done is not None:
            stream.wait_event(self._done)
        out = {"images": torch.empty((B,) + P + (C,), dtype=torch.float32, device=dev), "weights": torch.empty((B,) + P, dtype=torch.float32, device=dev),
               "labels": torch.empty((B,) + P + (K,), dtype=torch.float32, device=dev), "info": torch.empty((B + 1, 8), dtype=torch.int32, device=dev),
               "gamma": gamma}
        images, labels, weights, dims, n = self.c_tables()
        self.ctx.use_torch_stream()
        _lib.check(_lib.lib().ps_patch_sample_mixup_view(self.ctx.handle, images, labels, weights, dims, n, C, cand.ctypes.data_as(_lib.c_i32p), B, T,
                                                         (ctypes.c_int64 * 3)(*P), int(seed) & _M32, MODES[mode], K,
                                                         gamma.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), view, bits, runtime.ptr(out["images"]),
                                                         runtime.ptr(out["weights"]), runtime.ptr(out["labels"]), runtime.ptr(out["info"])))
        self._done = torch.cuda.Event()
        self._done.record(stream)
        return out

    def epoch_batches(self, batch_size, patch, epoch, seed=0, tries=8, rank=0, world=1, mode="one_positive", mixup=None, direction="axial", flip=None):
        """The batches of one epoch on one rank (epoch_plan), each drawn when the iterator reaches it.  mixup=K: mixed batches of batch_size
        slots, planned as epoch_plan(len(self), batch_size + 1, ...) -- the reference consumes B + 1 datapoints per mixed batch and then
        clears its holder.  direction and flip are sample's, the same for every batch (flip="random" draws from each batch's own seed)."""
        view = {} if direction == "axial" and flip is None else {"direction": direction, "flip": flip}  # (the defaults: today's call of sample)
        for _, cand, s in epoch_plan(len(self), batch_size + (0 if mixup is None else 1), epoch, seed, tries, rank, world):
            yield self.sample(cand, patch, s, mode, mixup, **view)


def train_saliency(net, bank, steps, patch, batch_size=2, lr=0.01, seed=0, epoch=0, optimizer=None, engine="autograd", dist=None, mixup=None,
                   direction="axial", flip=None):
    """The loop of train.py:83-110 on the device: `steps` steps on the bank's batches (epoch_batches from `epoch` on,
    config.DATA_SAMPLING = 'one_positive').  engine "autograd": TrainableSaliencyNet.loss under saliency.reference_optimizer(net, lr) (or
    `optimizer`); engine "native": net is a saliency.SaliencyTrainer and every step is one ps_saliency_train_step_prec at learning rate lr
    (dist: the torch.distributed-like module its gradients are summed through), at the precision the trainer was made with
    (SaliencyTrainer(precision=...): the trainer carries it, this loop takes no argument for it).  Returns the per-step losses as one device tensor
    [steps]; nothing is read back on the way.  mixup=num_classes: config.MIXUP, every batch is a mixed one (epoch_batches(mixup=...)) and
    the loss is dice_mixup's, on soft labels.  direction, flip: config.DIRECTION and sampler3d's flip, as PatchBank.sample takes them (patch
    in the view's axes; flip None, "random", or one 0 / 1 per drawn sample): the network trained with direction=view is the one
    saliency_map / evaluate_saliency take under that view's name."""
    from . import saliency
    if engine not in ("autograd", "native"):
        raise ValueError("train_saliency: engine must be 'autograd' or 'native'")
    native = engine == "native"
    if native and (not isinstance(net, saliency.SaliencyTrainer) or optimizer is not None):
        raise ValueError("train_saliency: the native engine takes a SaliencyTrainer and no optimizer")
    if not native and not isinstance(net, saliency.TrainableSaliencyNet):
        raise ValueError("train_saliency: net must be a TrainableSaliencyNet")
    if int(steps) < 1 or len(bank) < int(batch_size) + (0 if mixup is None else 1):
        raise ValueError("train_saliency: need steps >= 1 and at least batch_size volumes (one more with mixup) in the bank")
    if mixup is not None and int(mixup) != net.num_classes:
        raise ValueError("train_saliency: mixup must be the network's class count %d" % net.num_classes)
    if not native:
        opt = optimizer if optimizer is not None else saliency.reference_optimizer(net, lr)
    losses = []
    while len(losses) < steps:
        for batch in bank.epoch_batches(batch_size, patch, epoch, seed, mixup=mixup, direction=direction, flip=flip):
            if native:
                loss = net.step(batch["images"], batch["labels"], batch["weights"], lr, dist).clone()
            else:
                opt.zero_grad(set_to_none=True)
                loss = net.loss(batch["images"], batch["labels"], batch["weights"])
                loss.backward()
                opt.step()
            losses.append(loss.detach())
            if len(losses) == steps:
                break
        epoch += 1
    return torch.stack(losses)


def evaluate_saliency(bank, net, volumes, patch, steps, direction="axial", flip=False, batch=1):
    """EvalCallback / eval_pancreas: per volume c of `volumes`, saliency.saliency_map on the bank's image, its argmax, and binary_dice3d
    (utils.py:275-293: (2 s0 + 1e-10) / (s1 + s2 + 1e-10) with s0 = sum(pred * label), s1 = sum(pred), s2 = sum(label)) of the prediction
    against the label.  The three sums come from the device's confusion matrix (metrics.confusion: argmax with ties to the lowest index, as
    np.argmax): one read of num_classes^2 integers per volume.  net: a SaliencyNet, or a TrainableSaliencyNet (its weights are exported), or
    a dict of view name -> either, fused as saliency_map fuses it; direction, flip and batch are saliency_map's.  The image goes in as the
    bank keeps it, channels last.  Returns the list of Dice values (float)."""
    from . import metrics, saliency

    def exported(n):
        if isinstance(n, saliency.TrainableSaliencyNet):
            return saliency.SaliencyNet(n.export(), n.in_channels, n.num_classes, device=bank.device.index)
        return n

    net = {name: exported(n) for name, n in net.items()} if isinstance(net, dict) else exported(net)
    K = next(iter(net.values())).num_classes if isinstance(net, dict) else net.num_classes
    idx = np.arange(K, dtype=np.int64)
    out = []
    for c in volumes:
        image, label, _, _ = bank._vols[c]
        probs = saliency.saliency_map(image, net, patch, steps, direction=direction, flip=flip, batch=batch, layout="DHWC")
        cm = metrics.confusion(probs, label, K).cpu().numpy()  # rows truth, columns prediction
        s0 = int((cm * np.outer(idx, idx)).sum())
        s1, s2 = int((cm.sum(0) * idx).sum()), int((cm.sum(1) * idx).sum())
        out.append((2.0 * s0 + 1e-10) / (s1 + s2 + 1e-10))
    return out
