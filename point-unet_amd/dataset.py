"""Input side of the hot path: from a prepared .ply volume to the (xyz, features, labels, point index) tuple the network
consumes -- the generators of PointSegment/runBraTS.py:93-130 and runPancreas.py:96-118 as plain functions.

BraTS: all tumour voxels plus a uniform sample of background voxels up to cfg.num_points, shuffled (the shuffle is what
makes the later prefix slices `xyz[:, :N//r]` a random sub-sample, runBraTS.py:114,147).  Pancreas: the whole cloud in file
order.  Features are the reference's: xyz is concatenated in front of the modalities by tf_map (runBraTS.py:142).

sample_brats_cloud is the host form (numpy's generator).  CloudBank keeps a dataset's full clouds resident on the device and draws each
training batch there (ps_cloud_sample, csrc/cloud_sample.hip): the same distribution by a stated hash rule instead of numpy's stream."""
import collections
import ctypes

import numpy as np

from .helper_ply import read_ply

BRATS_MODALITIES = ("t1ce", "t1", "flair", "t2")  # runBraTS.py:105


def sample_brats_cloud(data, num_points, rng=None):
    """data: structured array with x, y, z, the four modalities and `class` (a prepared BraTS .ply).  Returns
    (xyz f32 [n,3], modalities f32 [n,4], labels, queried_idx i32 [n]) with n = max(num_points, #tumour voxels)."""
    rng = rng or np.random.default_rng()
    labels = np.asarray(data["class"])
    tumour = np.flatnonzero(labels > 0)
    background = np.flatnonzero(labels == 0)
    need = num_points - len(tumour)
    if need > len(background):
        raise ValueError("cloud has %d points, fewer than num_points = %d" % (len(labels), num_points))
    picked = rng.choice(background, size=max(need, 0), replace=False)
    idx = rng.permutation(np.concatenate([tumour, picked]))
    xyz = np.stack([data["x"], data["y"], data["z"]], axis=1)[idx].astype(np.float32)
    mods = np.stack([data[m] for m in BRATS_MODALITIES], axis=1)[idx].astype(np.float32)
    return xyz, mods, labels[idx], idx.astype(np.int32)


def pancreas_cloud(data):
    """data: structured array with x, y, z, value, class (a prepared Pancreas .ply): the whole cloud, file order."""
    xyz = np.stack([data["x"], data["y"], data["z"]], axis=1).astype(np.float32)
    value = np.asarray(data["value"], dtype=np.float32).reshape(-1, 1)
    return xyz, value, np.asarray(data["class"]), np.arange(len(xyz), dtype=np.int32)


def network_features(xyz, modalities):
    """tf_map's `features = concat(xyz, features)` (runBraTS.py:142)."""
    return np.concatenate([xyz, modalities], axis=-1).astype(np.float32)


def load_brats_ply(path, num_points, rng=None):
    return sample_brats_cloud(read_ply(path), num_points, rng)


def load_pancreas_ply(path):
    return pancreas_cloud(read_ply(path))


# ---- resident clouds, batches drawn on the device ---------------------------------------------------------------------------------------
_M32 = 0xFFFFFFFF


def _hash32(x):
    """lowbias32 on a Python int (the hash of ps_cloud_sample and of the training step's dropout)."""
    x &= _M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & _M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & _M32
    x ^= x >> 16
    return x


def batch_seed(seed, epoch, batch, rank=0):
    """The seed CloudBank.epoch_batches hands ps_cloud_sample for batch `batch` (0-based, counted over all ranks) of epoch `epoch` on
    rank `rank`: three rounds of hash32 over seed + 0x9E3779B9 (epoch + 1), + 0x85EBCA6B (batch + 1), + 0xC2B2AE35 (rank + 1), mod 2^32."""
    x = _hash32(seed + 0x9E3779B9 * (epoch + 1))
    x = _hash32(x + 0x85EBCA6B * (batch + 1))
    return _hash32(x + 0xC2B2AE35 * (rank + 1))


def epoch_plan(n_clouds, batch_size, epoch, seed=0, rank=0, world=1):
    """[(batch index, cloud ids, seed)] of one epoch on one rank, in the reference's order (runBraTS.py:82-97): clouds
    0 .. floor(n / bs) * bs - 1 in consecutive groups of batch_size; rank r of `world` takes batches r, r + world, ..."""
    bs, world, rank = int(batch_size), int(world), int(rank)
    if bs < 1 or world < 1 or not 0 <= rank < world:
        raise ValueError("epoch_plan: need batch_size >= 1 and 0 <= rank < world")
    n_batches = int(n_clouds) // bs
    return [(j, list(range(j * bs, (j + 1) * bs)), batch_seed(seed, epoch, j, rank)) for j in range(rank, n_batches, world)]


Batch = collections.namedtuple("Batch", "xyz features labels idx cloud_ids seed")
Batch.__doc__ = """One drawn batch (CUDA tensors): xyz f32 [B,N,3], features f32 [B,N,3+C] = [xyz | modalities], labels i32 [B,N],
idx i32 [B,N] (cloud-local rows: the reference's queried_idx, point2prod's p_idx); cloud_ids (list) and seed as drawn."""


class CloudBank:
    """A dataset's full clouds, resident on one GPU; training and validation batches drawn there by ps_cloud_sample.

    The reference's generator (runBraTS.py:91-130) reads a case's full cloud from its .ply, keeps every tumour point (label > 0), adds a
    uniform sample of background points without replacement up to cfg.num_points and shuffles (DP.shuffle_idx) -- the shuffle makes the
    pyramid's prefix slices a random subsample.  sample() draws the same distribution on the device from the bank's copy of every cloud,
    as a pure function of (cloud, labels, num_points, seed, slot) stated in include/pointseg.h: the same cloud in two slots gets two
    different samples, and equal arguments give the same batch bit for bit.  A training loop then never leaves HBM:

        bank = CloudBank(channels=4)
        for d in prepared_cases:                           # prepare.prepare_brats_volume(..., on_device=True) / read_ply arrays
            bank.add_prepared(d)
        pre = PyramidPrefetcher(cfg)
        trainer = Trainer(cfg)
        for epoch in range(epochs):
            batches = bank.epoch_batches(cfg.batch_size, cfg.num_points, epoch, seed=run_seed)
            cur = next(batches, None)
            if cur is not None:
                pre.submit(cur.xyz)
            while cur is not None:
                nxt = next(batches, None)                  # drawn on the caller's stream, behind the step enqueued last
                if nxt is not None:
                    pre.submit(nxt.xyz)                    # its pyramid is built on the prefetch stream under this step
                pyr, slot = pre.next()
                loss = trainer.train_step(pyr, cur.features, cur.labels)
                pre.release(slot)
                cur = nxt
        bank.synchronize()                                 # raises if a stale positive count was found on the device

    Validation: metrics.validate(net, ((build_pyramid(b.xyz, cfg), b.features, b.labels) for b in batches)), and
    postprocess.point2prod(logits[k], b.idx[k], bank.origin(b.cloud_ids[k])) for the volume of slot k.

    Memory: rows of all clouds in three device arrays (xyz, modalities, int32 labels) grown by doubling, plus each cloud's xyz_origin.
    Streams: every call runs on torch's current stream; consecutive calls on different streams are ordered through an event (they share
    the context's workspace).  The bank's own context (ctx=None) validates the device's positive counts without synchronising
    (ps_set_deferred_checks): a disagreement surfaces at synchronize()."""

    def __init__(self, channels=4, device=0, ctx=None):
        import torch

        from . import runtime
        self.channels = int(channels)
        if not 1 <= self.channels <= 16:
            raise ValueError("CloudBank: channels must be in [1, 16]")
        self.device = torch.device("cuda", int(device))
        if ctx is None:
            ctx = runtime.Context(self.device.index)
            ctx.set_deferred_checks(True)
        self.ctx = ctx
        self._offsets = [0]
        self._positives = []
        self._origins = []
        self._labelled = False
        self._xyz = torch.empty((0, 3), dtype=torch.float32, device=self.device)
        self._mods = torch.empty((0, self.channels), dtype=torch.float32, device=self.device)
        self._labels = torch.empty(0, dtype=torch.int32, device=self.device)
        self._done = None  # event behind the last sample(): the next one may run on another stream but reuses the workspace

    def __len__(self):
        return len(self._offsets) - 1

    @property
    def total_points(self):
        return self._offsets[-1]

    def num_points(self, c):
        return self._offsets[c + 1] - self._offsets[c]

    def positives(self, c):
        """Points with label > 0 in cloud c (counted on the device when it was added)."""
        return int(self._positives[c])

    def origin(self, c):
        """xyz_origin of cloud c (int32 [n, 3] CUDA tensor, voxel coordinates for postprocess.point2prod), or None."""
        return self._origins[c]

    def _dev(self, a, dtype):
        import torch
        t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
        return t.to(device=self.device, dtype=dtype).contiguous()

    def _grow(self, need):
        import torch
        cap = self._xyz.shape[0]
        if need <= cap:
            return
        new = max(need, 2 * cap, 1 << 16)
        n = self.total_points
        for name, shape, dtype in (("_xyz", (new, 3), torch.float32), ("_mods", (new, self.channels), torch.float32), ("_labels", (new,), torch.int32)):
            t = torch.zeros(shape, dtype=dtype, device=self.device)
            t[:n] = getattr(self, name)[:n]
            setattr(self, name, t)

    def add(self, xyz, modalities, labels=None, xyz_origin=None):
        """One full cloud: xyz [n, 3], modalities [n, channels], labels [n] integer or None (all background), xyz_origin [n, 3] or None;
        numpy arrays or CUDA tensors.  Returns the cloud id (0, 1, ... in order of adding).  Not the hot path: one synchronisation."""
        import torch

        from . import _lib, runtime
        xyz = self._dev(xyz, torch.float32)
        mods = self._dev(modalities, torch.float32)
        n = xyz.shape[0]
        if xyz.dim() != 2 or xyz.shape[1] != 3:
            raise ValueError("CloudBank.add: xyz must have shape [n, 3]")
        if tuple(mods.shape) != (n, self.channels):
            raise ValueError("CloudBank.add: modalities must have shape [%d, %d], got %s" % (n, self.channels, tuple(mods.shape)))
        if not 1 <= n < (1 << 31):
            raise ValueError("CloudBank.add: a cloud holds 1 to 2^31 - 1 points")
        lab = None
        if labels is not None:
            lab = self._dev(labels, torch.int32).reshape(-1)
            if lab.numel() != n:
                raise ValueError("CloudBank.add: %d labels for %d points" % (lab.numel(), n))
        org = None
        if xyz_origin is not None:
            org = self._dev(xyz_origin, torch.int32)
            if tuple(org.shape) != (n, 3):
                raise ValueError("CloudBank.add: xyz_origin must have shape [n, 3]")
        r0 = self.total_points
        self._grow(r0 + n)
        self._xyz[r0:r0 + n] = xyz
        self._mods[r0:r0 + n] = mods
        count = 0
        if lab is not None:
            self._labels[r0:r0 + n] = lab
            self._labelled = True
            off = (ctypes.c_int64 * 2)(0, n)
            cnt = (ctypes.c_int64 * 1)()
            self.ctx.use_torch_stream()
            _lib.check(_lib.lib().ps_cloud_positive_counts(self.ctx.handle, runtime.ptr(self._labels[r0:r0 + n]), off, 1, cnt))
            count = int(cnt[0])
        else:
            self._labels[r0:r0 + n] = 0
        self._offsets.append(r0 + n)
        self._positives.append(count)
        self._origins.append(org)
        return len(self) - 1

    def add_ply_data(self, data):
        """A prepared BraTS .ply as read_ply returns it (x, y, z, t1ce, t1, flair, t2, class): the generator's full cloud
        (runBraTS.py:98-101)."""
        xyz = np.stack([data["x"], data["y"], data["z"]], axis=1).astype(np.float32)
        mods = np.stack([data[m] for m in BRATS_MODALITIES], axis=1).astype(np.float32)
        labels = np.asarray(data["class"]).astype(np.int32) if "class" in data.dtype.names else None
        return self.add(xyz, mods, labels)

    def add_prepared(self, d):
        """The full-cloud arrays of prepare.prepare_brats_volume (xyz, colors, labels, xyz_origin; numpy, or CUDA tensors with
        on_device=True)."""
        return self.add(d["xyz"], d["colors"], d.get("labels"), d.get("xyz_origin"))

    def sample(self, cloud_ids, num_points, seed=0):
        """One batch of len(cloud_ids) slots x num_points points, drawn on the device (ps_cloud_sample) on torch's current stream.
        Returns a Batch of CUDA tensors, ready for build_pyramid / PyramidPrefetcher.submit (xyz), Trainer.train_step (features, labels),
        metrics.validate and postprocess.point2prod (idx)."""
        import torch

        from . import _lib, runtime
        ids = np.ascontiguousarray(np.asarray(cloud_ids, dtype=np.int64).reshape(-1))
        if ids.size and (ids.min() < 0 or ids.max() >= len(self)):
            raise ValueError("CloudBank.sample: cloud ids must be in [0, %d)" % len(self))
        ids = ids.astype(np.int32)
        B, N, C = len(ids), int(num_points), self.channels
        off = (ctypes.c_int64 * len(self._offsets))(*self._offsets)
        pos = (ctypes.c_int64 * max(len(self._positives), 1))(*self._positives)
        cid = (ctypes.c_int32 * max(B, 1))(*ids.tolist())
        dev = self.device
        stream = torch.cuda.current_stream(dev)
        if self._done is not None:
            stream.wait_event(self._done)
        xyz = torch.empty((B, N, 3), dtype=torch.float32, device=dev)
        feats = torch.empty((B, N, 3 + C), dtype=torch.float32, device=dev)
        labels = torch.empty((B, N), dtype=torch.int32, device=dev)
        idx = torch.empty((B, N), dtype=torch.int32, device=dev)
        self.ctx.use_torch_stream()
        lab = self._labels if self._labelled else None
        _lib.check(_lib.lib().ps_cloud_sample(self.ctx.handle, runtime.ptr(self._xyz), runtime.ptr(self._mods), C, runtime.ptr(lab), off, len(self), pos,
                                              cid, B, N, int(seed) & _M32, runtime.ptr(xyz), runtime.ptr(feats), runtime.ptr(labels), runtime.ptr(idx)))
        self._done = torch.cuda.Event()
        self._done.record(stream)
        return Batch(xyz, feats, labels, idx, ids.tolist(), int(seed) & _M32)

    def epoch_batches(self, batch_size, num_points, epoch, seed=0, rank=0, world=1):
        """The batches of one epoch on one rank, each drawn when the iterator reaches it: epoch_plan's order (the reference's: clouds
        0 .. floor(n / bs) * bs - 1 in groups of batch_size, runBraTS.py:82-97; rank r takes every world-th batch) and
        batch_seed(seed, epoch, batch, rank) as each batch's seed."""
        for _, ids, s in epoch_plan(len(self), batch_size, epoch, seed, rank, world):
            yield self.sample(ids, num_points, s)

    def synchronize(self):
        """Wait for the bank's work and raise a deferred error (a stale positive count) if the device found one."""
        self.ctx.synchronize()
