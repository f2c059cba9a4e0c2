"""The device kd-tree builder (csrc/kdtree_build.hip) at every node-size tier, alone and in sets, against the product's host builder
(csrc/kdtree_host.hip, itself held to the oracle's tree at these sizes by tests/test_kdtree_tier_coverage.py).  Every comparison is exact:
permutation, point records, root, depth, box, the node tables walked from the root, and the three-record image the searches read.  Each
case also proves that its branch ran: the counters the builder leaves behind (csrc/debug_hooks.h: ps_debug_kdtree_device_set) are compared
with a census of the HOST tree (kdtree_cases.census), never with a second device run."""
import time

import numpy as np
import pytest

import kdtree_cases as kc

pytestmark = pytest.mark.gpu


def _ctx():
    from point_unet_amd import runtime
    return runtime.default_context(0)


def _check_set(lib, dbg, cases, want_copy=None):
    """Builds the set on the device and holds every tree, its fat image and the counters to the host builder's trees; returns the device
    run (trees, copies, stats) and the expected counters."""
    host = kc.host_trees(dbg, cases)
    trees, copies, stats = kc.device_set(lib, dbg, _ctx(), cases, want_copy)
    for case, h, d in zip(cases, host, trees):
        what = "%s n=%d seed=%d" % case
        inner = kc.assert_same_tree(h, d, what)
        kc.assert_fat_image(d, inner, what)
    want = kc.expected_stats([kc.census(h) for h in host], max(c[1] for c in cases))
    assert stats[kc.S_FLAG0] == 0 and stats[kc.S_FLAG1] == 0, stats
    assert np.array_equal(stats, want), "builder counters %s != census of the host trees %s" % (stats.tolist(), want.tolist())
    return trees, copies, stats, want


@pytest.mark.parametrize("n", kc.SINGLE_SIZES)
def test_single_trees_at_every_switch(lib, dbg, n):
    """(a) one tree per plan, on both sides of kLeafMax, kSmall, kSlab, kChunk, kMid = kHuge and of every further chunked level, in all five
    cloud variants."""
    k = kc.constants()
    for case in kc.single_cases():
        if case[1] != n:
            continue
        _, _, stats, _ = _check_set(lib, dbg, [case])
        levels = 0 if n <= k["kMid"] else 1 if n <= 2 * k["kMid"] else 2 if n <= 4 * k["kMid"] else 3
        assert stats[kc.S_LEVELS] == levels, (case, stats)
        if n == k["kMid"] + 1:  # one task of three chunks: kChunk, kChunk, 1
            assert stats[kc.S_NTASKS] == 1 and stats[kc.S_NCHUNKS] == 3 and stats[kc.S_NTASKS + 1] == 0, (case, stats)
        if n <= k["kSmall"]:
            assert stats[kc.S_MID] == 0 and stats[kc.S_SMALL] == 1, (case, stats)
        if n == k["kSmall"] + 1:
            assert stats[kc.S_MID] == 1, (case, stats)
        if n <= k["kMid"]:
            assert not stats[kc.S_NTASKS:kc.S_STRAGGLERS + 1].any(), (case, stats)


def _mixed_copy():
    return [i % 2 for i in range(len(kc.MIXED_SET))]


def test_mixed_set(lib, dbg):
    """(b) trees of every tier in ONE plan: the five chunked levels the largest tree asks for are applied to all of them, and each tree
    still equals its own single-tree host build; the copied source rows arrive where they were asked for."""
    k = kc.constants()
    wc = _mixed_copy()
    trees, copies, stats, want = _check_set(lib, dbg, kc.MIXED_SET, wc)
    assert stats[kc.S_LEVELS] == 5
    for case, w, rows in zip(kc.MIXED_SET, wc, copies):
        assert (rows is not None) == bool(w)
        if w:
            assert np.array_equal(rows.view(np.int32), kc.cloud(*case).view(np.int32)), case
    # only the trees above kMid have chunked tasks: 70 000 uniform, 4 097 lattice5, 30 005 outliers, 8 193 identical
    roots = [c for c in kc.MIXED_SET if c[1] > k["kHuge"]]
    assert stats[kc.S_NTASKS] == len(roots) == 4
    assert stats[kc.S_NCHUNKS] == sum(-(-c[1] // k["kChunk"]) for c in roots)
    assert stats[kc.S_NTASKS:kc.S_NTASKS + 5].all() and not stats[kc.S_NTASKS + 5:kc.S_NCHUNKS].any()


def test_many_roots(lib, dbg):
    """(c) 300 trees in one plan: huge_root_kernel's loop over the roots goes past its 256 threads."""
    assert len(kc.MANY_ROOTS) > 256
    _, _, stats, _ = _check_set(lib, dbg, kc.MANY_ROOTS)
    k = kc.constants()
    assert stats[kc.S_LEVELS] == 0 and stats[kc.S_MID] == sum(c[1] > k["kSmall"] for c in kc.MANY_ROOTS) == 44


def test_more_than_256_chunked_tasks_in_a_level(lib, dbg):
    """(d) three 600 000-point trees: 384 tasks at the last chunked level, huge_plan_block's second round and its carry (the census is
    re-asserted on the CPU: tests/test_kdtree_tier_coverage.py)."""
    k = kc.constants()
    kc.host_trees(dbg, kc.PLAN_ROUNDS_SET)
    t0 = time.perf_counter()
    _, _, stats, _ = _check_set(lib, dbg, kc.PLAN_ROUNDS_SET)
    print("(d) device build of 3 x 600 000 points + exact comparison: %.2f s" % (time.perf_counter() - t0))
    last = k["kHugeLevels"] - 1
    assert stats[kc.S_LEVELS] == k["kHugeLevels"] and stats[kc.S_NTASKS + last] == 384 > 256
    assert stats[kc.S_NTASKS:kc.S_NTASKS + 8].tolist() == [3 << d for d in range(8)]


def test_stragglers_on_a_balanced_tree(lib, dbg):
    """(e) 1 100 000 points: after all eight chunked levels 256 nodes are still above kMid and go to build_level_kernel."""
    k = kc.constants()
    kc.host_trees(dbg, kc.STRAGGLER_SET)
    t0 = time.perf_counter()
    _, _, stats, _ = _check_set(lib, dbg, kc.STRAGGLER_SET)
    print("(e) device build of 1 100 000 points + exact comparison: %.2f s" % (time.perf_counter() - t0))
    assert stats[kc.S_LEVELS] == k["kHugeLevels"] and stats[kc.S_STRAGGLERS] == 256
    assert stats[kc.S_MID] == 512  # each of them splits once into two mid-queue nodes


def test_two_runs_of_the_mixed_set_are_byte_equal(lib, dbg):
    """(f) every returned array, unreached slots included: the build is a function of its input, not of scheduling.  (The arena hands the
    second run the first one's memory, so a slot that no kernel writes holds the first run's value.)"""
    runs = []
    for _ in range(2):
        trees, copies, stats = kc.device_set(lib, dbg, _ctx(), kc.MIXED_SET, _mixed_copy())
        runs.append(([getattr(t, f).tobytes() for t in trees for f in kc.Tree.FIELDS + ("fat",)], [c.tobytes() for c in copies if c is not None],
                     stats.tobytes()))
    assert runs[0] == runs[1]
