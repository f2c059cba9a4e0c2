"""Clouds, host trees and tree arithmetic shared by the tests of the device kd-tree builder's size tiers (tests/test_gpu_kdtree_tiers.py on
the kernels, tests/test_kdtree_tier_coverage.py on the CPU).  csrc/kdtree_build.hip picks a code path by node size; the sizes below sit on
every switch, and census() says from a HOST tree alone which path each node of it takes, so that a GPU test can prove that its branch ran
by comparing the builder's counters (csrc/debug_hooks.h: ps_debug_kdtree_device_set) with numbers no device run produced.

Every cloud and every host tree is made once per session and handed out read-only."""
import ctypes
import functools
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "point-unet_amd", "csrc")

VARIANTS = ("uniform", "lattice5", "identical", "line", "outliers")
# (a) single trees at every switch: kLeafMax, kSmall, kSlab, kChunk, kMid = kHuge, each with its neighbours; 1 024 / 1 025 (build_mid_kernel's
# thread count), 6 143..6 145 (three chunks to the last record), 2 kMid +- 1 and 4 kMid + 1 (a further chunked level each), 3 kMid + 1
SINGLE_SIZES = [1, 2, 9, 10, 11, 20, 21, 255, 256, 257, 511, 512, 513, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 6143, 6144, 6145, 8191, 8192, 8193,
                12289, 16385]
OUTLIERS_MIN_N = 50
# (b) one plan of unlike trees: (variant, n, seed)
MIXED_SET = [("uniform", 70000, 31), ("lattice5", 4097, 32), ("line", 4096, 33), ("identical", 257, 34), ("uniform", 256, 35), ("uniform", 11, 36),
             ("uniform", 10, 37), ("uniform", 1, 38), ("outliers", 30005, 39), ("identical", 8193, 40)]
# (c) more roots than huge_root_kernel has threads
MANY_ROOTS = [("lattice5", n, 100 + n) for n in range(1, 301)]
# (d) more than 256 chunked tasks in one level: huge_plan_block's second round
PLAN_ROUNDS_SET = [("uniform", 600000, 51), ("uniform", 600000, 52), ("uniform", 600000, 53)]
# (e) a balanced tree whose nodes are still above kMid after every chunked level
STRAGGLER_SET = [("uniform", 1100000, 61)]

REF_ID_MASK = (1 << 26) - 1  # csrc/kdtree.h: kRefIdMask
N_STATS = 22                 # csrc/debug_hooks.h: PS_DEBUG_KDTREE_STATS
S_LEVELS, S_NTASKS, S_NCHUNKS, S_STRAGGLERS, S_MID, S_SMALL, S_FLAG0, S_FLAG1 = 0, 1, 9, 17, 18, 19, 20, 21


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def constants(build_src=None, tree_src=None):
    """{name: value} of the builder's size switches, parsed from the sources (a value may name an earlier constant: kHuge = kMid)."""
    build_src = build_src if build_src is not None else open(os.path.join(CSRC, "kdtree_build.hip")).read()
    tree_src = tree_src if tree_src is not None else open(os.path.join(CSRC, "kdtree.h")).read()
    out = {}
    for src, names in ((tree_src, ("kLeafMax",)), (build_src, ("kSmall", "kMid", "kSlab", "kHuge", "kHugeLevels", "kChunk"))):
        for name in names:
            m = re.findall(r"^constexpr int %s = ([^;]+);" % name, src, re.M)
            assert len(m) == 1, "constexpr int %s: %d definitions found" % (name, len(m))
            out[name] = int(eval(m[0], {"__builtins__": {}}, dict(out)))
    return out


# ---- clouds ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cloud(variant, n, seed):
    """uniform: no ties.  lattice5: coordinates 0, 1/4 .. 1 -- at most 125 distinct points, every cut a lattice plane, many records equal to
    it.  identical: n copies of one point, every record equals every cut.  line: the shuffled geometric progression r^i on x (r = 0.97 up to
    1 200 points, 1 - 700 / n above: a bounding-box-midpoint split peels n ln2 / 700 points off, most levels stay lopsided, and the tail that
    underflows fp32 is one run of zeros).  outliers: n - 5 uniform points and 5 at +100, the big child's midpoint lies outside its records."""
    rng = np.random.default_rng(seed)
    if variant == "uniform":
        p = rng.random((n, 3), dtype=np.float32)
    elif variant == "lattice5":
        p = (rng.integers(0, 5, size=(n, 3)) / 4.0).astype(np.float32)
    elif variant == "identical":
        p = np.repeat(rng.random((1, 3), dtype=np.float32), n, axis=0)
    elif variant == "line":
        r = 0.97 if n <= 1200 else 1.0 - 700.0 / n
        p = np.stack([r ** np.arange(n), np.zeros(n), np.zeros(n)], 1).astype(np.float32)[rng.permutation(n)]
    elif variant == "outliers":
        assert n >= OUTLIERS_MIN_N
        p = np.concatenate([rng.random((n - 5, 3), dtype=np.float32), 100 + rng.random((5, 3), dtype=np.float32)])[rng.permutation(n)]
    else:
        raise KeyError(variant)
    assert p.shape == (n, 3) and p.dtype == np.float32
    return _frozen(p)


def single_cases():
    """[(variant, n, seed)] of (a)."""
    return [(v, n, 7 + i) for n in SINGLE_SIZES for i, v in enumerate(VARIANTS) if not (v == "outliers" and n < OUTLIERS_MIN_N)]


# ---- trees ----------------------------------------------------------------------------------------------------------------------------
class Tree:
    """The arrays of ps_debug_kdtree_host / ps_debug_kdtree_device for one tree."""
    FIELDS = ("vind", "nodes", "pts", "root_depth", "bbox")

    def __init__(self, n, **arrays):
        self.n = n
        for f in self.FIELDS:
            setattr(self, f, arrays[f])
        self.fat = arrays.get("fat")

    @property
    def root(self):
        return int(self.root_depth[0])


def _empty(n):
    return dict(vind=np.zeros(n, np.int32), nodes=np.zeros((2 * n, 4), np.int32), pts=np.zeros((n, 4), np.float32), root_depth=np.zeros(2, np.int32),
                bbox=np.zeros(6, np.float32))


def bind_host(dbg):
    c_vp = ctypes.c_void_p
    dbg.ps_debug_kdtree_host.restype = ctypes.c_int
    dbg.ps_debug_kdtree_host.argtypes = [c_vp, ctypes.c_int64, c_vp, c_vp, c_vp, c_vp, c_vp]


def bind_device_set(dbg):
    c_vp = ctypes.c_void_p
    dbg.ps_debug_kdtree_device_set.restype = ctypes.c_int
    dbg.ps_debug_kdtree_device_set.argtypes = [c_vp, c_vp, c_vp, ctypes.c_int64] + [c_vp] * 9


_host_trees = {}


def host_tree(dbg, variant, n, seed):
    """The product's host builder (csrc/kdtree_host.hip) on cloud(variant, n, seed): one ps_debug_kdtree_host call, cached."""
    key = (variant, n, seed)
    if key not in _host_trees:
        bind_host(dbg)
        p = cloud(*key)
        a = _empty(n)
        assert dbg.ps_debug_kdtree_host(p.ctypes.data, n, *[a[f].ctypes.data for f in Tree.FIELDS]) == 0
        _host_trees[key] = Tree(n, **{f: _frozen(v) for f, v in a.items()})
    return _host_trees[key]


def host_trees(dbg, cases):
    return [host_tree(dbg, *c) for c in cases]


def device_set(lib, dbg, ctx, cases, want_copy=None):
    """One ps_debug_kdtree_device_set call over the clouds of `cases`: ([Tree with .fat], copy rows per tree or None, stats)."""
    bind_device_set(dbg)
    ns = np.array([c[1] for c in cases], np.int32)
    sup = np.ascontiguousarray(np.concatenate([cloud(*c) for c in cases]))
    tot, T = int(ns.sum()), len(cases)
    wc = np.zeros(T, np.int32) if want_copy is None else np.asarray(want_copy, np.int32)
    vind, nodes, pts, fat = np.zeros(tot, np.int32), np.zeros((2 * tot, 4), np.int32), np.zeros((tot, 4), np.float32), np.zeros((6 * tot, 4), np.int32)
    rd, bbox, stats = np.zeros((T, 2), np.int32), np.zeros((T, 6), np.float32), np.full(N_STATS, -1, np.int32)
    copy = np.full((int(ns[wc != 0].sum()) + 1, 3), np.nan, np.float32)
    rc = dbg.ps_debug_kdtree_device_set(ctx.handle, sup.ctypes.data, ns.ctypes.data, T, wc.ctypes.data, vind.ctypes.data, nodes.ctypes.data,
                                        pts.ctypes.data, fat.ctypes.data, rd.ctypes.data, bbox.ctypes.data, copy.ctypes.data, stats.ctypes.data)
    assert rc == 0, lib.ps_last_error()
    trees, copies, o, oc = [], [], 0, 0
    for i, n in enumerate(int(v) for v in ns):
        trees.append(Tree(n, vind=vind[o:o + n], nodes=nodes[2 * o:2 * (o + n)], pts=pts[o:o + n], root_depth=rd[i], bbox=bbox[i], fat=fat[6 * o:6 * (o + n)]))
        copies.append(copy[oc:oc + n] if wc[i] else None)
        o, oc = o + n, oc + (n if wc[i] else 0)
    assert np.isnan(copy[oc:]).all(), "the door wrote past the copy rows it was asked for"
    return trees, copies, stats


# ---- walking a node table (layout: csrc/kdtree.h) ---------------------------------------------------------------------------------------
def walk_levels(nodes, root, n):
    """Depth by depth from the root: (depth, ids, lo, hi, parent sizes) of the nodes at that depth, as arrays.  A node covers vind positions
    [lo, hi); an inner node has an odd id 2 m - 1 and children [lo, m), [m, hi); the root's parent size is 0."""
    ref, lo, hi, par = np.array([root], np.int64), np.array([0], np.int64), np.array([n], np.int64), np.array([0], np.int64)
    depth = 0
    while len(ref):
        ids = ref & REF_ID_MASK
        assert ((ids >= 0) & (ids < 2 * n)).all(), "a child reference leaves the node table"
        yield depth, ids, lo, hi, par
        inner = (ids & 1) == 1
        ii, l, h = ids[inner], lo[inner], hi[inner]
        m = (ii + 1) // 2
        assert ((l < m) & (m < h)).all(), "an inner node's split position lies outside its range"
        c1, c2 = nodes[ii, 0].astype(np.int64) & 0x3fffffff, nodes[ii, 1].astype(np.int64)
        ref = np.stack([c1, c2], 1).reshape(-1)
        lo, hi = np.stack([l, m], 1).reshape(-1), np.stack([m, h], 1).reshape(-1)
        par = np.repeat(h - l, 2)
        depth += 1
        assert depth <= 2 * n + 2, "the node table has a cycle"


def assert_same_nodes(want, got, what=""):
    """The node records of `got` equal those of `want` at every id reached from want's root (unreached slots are unspecified); whole
    levels at a time.  Returns the ids of the inner nodes."""
    assert want.n == got.n and int(got.root_depth[0]) == want.root, what
    inner_ids = []
    for depth, ids, lo, hi, _ in walk_levels(want.nodes, want.root, want.n):
        bad = np.flatnonzero((want.nodes[ids] != got.nodes[ids]).any(1))
        assert len(bad) == 0, "%s depth %d: %d of %d node records differ, first id %d: %s != %s" % (
            what, depth, len(bad), len(ids), ids[bad[0]], got.nodes[ids[bad[0]]], want.nodes[ids[bad[0]]])
        inner_ids.append(ids[(ids & 1) == 1])
    return np.concatenate(inner_ids)


def assert_same_tree(want, got, what=""):
    """Everything exact: permutation, point records (bit for bit), root, depth, box, and the node tables from the root."""
    assert np.array_equal(want.vind, got.vind), "%s: vind permutation differs" % what
    assert np.array_equal(want.pts.view(np.int32), got.pts.view(np.int32)), "%s: point records differ" % what
    assert np.array_equal(want.root_depth, got.root_depth), "%s: root / depth %s != %s" % (what, got.root_depth, want.root_depth)
    assert np.array_equal(want.bbox.view(np.int32), got.bbox.view(np.int32)), "%s: bounding box differs" % what
    return assert_same_nodes(want, got, what)


def assert_fat_image(tree, inner_ids, what=""):
    """fat[3 id] = nodes[id] for every reachable inner id; fat[3 id + 1] / [3 id + 2] = the record of the first / second child where that
    child is an inner node (fatten_kernel leaves zeros for a leaf child, which the search never reads: not asserted)."""
    ids = inner_ids
    assert np.array_equal(tree.fat[3 * ids], tree.nodes[ids]), "%s: fat[3 id] != nodes[id]" % what
    for k, child in ((1, tree.nodes[ids, 0] & 0x3fffffff), (2, tree.nodes[ids, 1])):
        cid = child & REF_ID_MASK
        sel = (cid & 1) == 1
        assert np.array_equal(tree.fat[3 * ids[sel] + k], tree.nodes[cid[sel]]), "%s: fat[3 id + %d] != nodes[child]" % (what, k)


# ---- which path every node of a host tree takes -------------------------------------------------------------------------------------------
def census(tree, k=None):
    """From a finished (host) tree: big[d] = sizes of the nodes at depth d with more than kMid (= kHuge) points, in walk order; chunks[d] =
    their ceil(size / kChunk); mid = nodes of kSmall + 1 .. kMid points that are roots or whose parent is above kMid (what is pushed to
    build_mid_kernel's queue); small = nodes of at most kSmall points, leaves included, that are roots or whose parent is above kSmall
    (build_flat_kernel's queue)."""
    k = k or constants()
    assert k["kHuge"] == k["kMid"]
    big, chunks, mid, small = {}, {}, 0, 0
    for depth, ids, lo, hi, par in walk_levels(tree.nodes, tree.root, tree.n):
        size = hi - lo
        top = par == 0
        b = size[size > k["kMid"]]
        if len(b):
            big[depth] = b
            chunks[depth] = (b + k["kChunk"] - 1) // k["kChunk"]
        mid += int(((size > k["kSmall"]) & (size <= k["kMid"]) & (top | (par > k["kMid"]))).sum())
        small += int(((size <= k["kSmall"]) & (top | (par > k["kSmall"]))).sum())
    return dict(big=big, chunks=chunks, mid=mid, small=small)


def chunked_levels(max_n, k=None):
    """The chunked levels the host launches for a set whose largest tree has max_n points: min(kHugeLevels, ceil(log2(max_n / kMid)))."""
    k = k or constants()
    levels = 0
    while levels < k["kHugeLevels"] and max_n > (k["kMid"] << levels):
        levels += 1
    return levels


def expected_stats(censuses, max_n, k=None):
    """The counters of ps_debug_kdtree_device_set (csrc/debug_hooks.h) for a set of trees, from their censuses."""
    k = k or constants()
    L = chunked_levels(max_n, k)
    s = np.zeros(N_STATS, np.int32)
    s[S_LEVELS] = L
    for c in censuses:
        for d in range(L):
            s[S_NTASKS + d] += len(c["big"].get(d, ()))
            s[S_NCHUNKS + d] += int(np.sum(c["chunks"].get(d, ())))
        s[S_STRAGGLERS] += len(c["big"].get(L, ()))
        s[S_MID] += c["mid"]
        s[S_SMALL] += c["small"]
    return s


# ---- the host builder against the oracle's tree -------------------------------------------------------------------------------------------
def assert_oracle_top(tree, p, t):
    """Permutation, box and point records against oracle.kdtree_export's."""
    assert np.array_equal(tree.vind, t["vind"])
    assert np.array_equal(tree.bbox, t["bbox"])
    assert np.array_equal(tree.pts[:, :3], p[tree.vind]) and np.array_equal(tree.pts[:, 3].view(np.int32), tree.vind)


def assert_oracle_tree(tree, p, t):
    """Same permutation, same splits, same child order as the oracle's tree t = oracle.kdtree_export(p), in the product's id scheme."""
    assert_oracle_top(tree, p, t)
    nodes, n = tree.nodes, tree.n

    def walk(oid, ref, lo, hi):
        pid, cnt = ref & ((1 << 26) - 1), ref >> 26  # reference = node id | leaf point count << 26 (csrc/kdtree.h)
        if t["axis"][oid] < 0:
            assert cnt == hi - lo and pid % 2 == 0 and pid // 2 == t["a"][oid] == lo and nodes[pid, 0] == lo and nodes[pid, 1] == t["b"][oid] == hi
            return 1
        assert cnt == 0 and pid % 2 == 1
        m = (pid + 1) // 2
        ax = (int(nodes[pid, 0]) & 0xffffffff) >> 30
        assert ax == t["axis"][oid]
        assert nodes[pid, 2:].view(np.float32)[0] == t["lo"][oid] and nodes[pid, 2:].view(np.float32)[1] == t["hi"][oid]
        c1, c2 = int(nodes[pid, 0]) & 0x3fffffff, int(nodes[pid, 1])
        return 1 + max(walk(t["a"][oid], c1, lo, m), walk(t["b"][oid], c2, m, hi))

    depth = walk(0, int(tree.root_depth[0]), 0, n)
    assert depth - 1 == tree.root_depth[1]
