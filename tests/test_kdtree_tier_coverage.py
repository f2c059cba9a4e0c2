"""The device kd-tree builder (csrc/kdtree_build.hip) picks a kernel by node size: leaves up to kLeafMax, build_flat_kernel up to kSmall,
build_mid_kernel up to kMid in slabs of kSlab, the chunked levels above kHuge = kMid in chunks of kChunk for at most kHugeLevels levels,
build_level_kernel for what is still above kMid after them.  tests/test_gpu_kdtree_tiers.py runs the builder on every side of every
switch; these CPU tests hold its size list and the censuses its large cases rest on to the constants in the sources, so that a retuned
constant fails here, saying which sizes to move, instead of silently un-covering a tier -- and they hold the yardstick of all of it, the
product's host builder, to the oracle's tree at every one of those sizes."""
import numpy as np
import pytest

import kdtree_cases as kc

EXPECTED = dict(kLeafMax=10, kSmall=256, kMid=4096, kHuge=4096, kSlab=512, kChunk=2048, kHugeLevels=8)


def _missing_sizes(sizes, k):
    """[(what, the sizes it wants that the list lacks)]: every switch with its two neighbours, the chunked-level edges 2 kMid and 4 kMid + 1."""
    want = [(name, [k[name] - 1, k[name], k[name] + 1]) for name in ("kLeafMax", "kSmall", "kSlab", "kChunk", "kMid", "kHuge")]
    want += [("2 kMid (last size of one chunked level)", [2 * k["kMid"]]), ("4 kMid + 1 (first size of three chunked levels)", [4 * k["kMid"] + 1])]
    return [(name, sorted(set(v) - set(sizes))) for name, v in want if set(v) - set(sizes)]


def test_the_constants_parse_and_are_what_the_cases_were_chosen_for():
    k = kc.constants()
    assert k == EXPECTED, "a size switch of kdtree_build.hip moved: re-derive kdtree_cases.SINGLE_SIZES and the sets (d) and (e) (%s)" % k


def test_the_single_tree_sizes_sit_on_every_switch():
    missing = _missing_sizes(kc.SINGLE_SIZES, kc.constants())
    assert missing == [], "kdtree_cases.SINGLE_SIZES lacks sizes next to a switch -- add them: %s" % missing
    assert kc.SINGLE_SIZES == sorted(set(kc.SINGLE_SIZES))
    # the chunked levels of those sizes, as test (a) expects them: 0 up to kMid, one more at every doubling
    k = kc.constants()
    assert [kc.chunked_levels(n) for n in (k["kMid"], k["kMid"] + 1, 2 * k["kMid"], 2 * k["kMid"] + 1, 4 * k["kMid"], 4 * k["kMid"] + 1)] == [0, 1, 1, 2, 2, 3]
    assert kc.chunked_levels(1 << 24) == k["kHugeLevels"]
    # every variant at every size, the outliers from 50 points on
    cases = kc.single_cases()
    assert len(cases) == len(set(cases)) == sum(len(kc.VARIANTS) - (n < kc.OUTLIERS_MIN_N) for n in kc.SINGLE_SIZES)


def test_the_guard_sees_a_removed_size_and_a_moved_constant():
    k = kc.constants()
    for gone, name in ((4097, "kMid"), (257, "kSmall")):
        bad = _missing_sizes([n for n in kc.SINGLE_SIZES if n != gone], k)
        assert bad and all(gone in sizes for _, sizes in bad) and name in [b[0] for b in bad], (gone, bad)
    # a retuned constant: the parser follows the source, the guard names the sizes to add
    src = open(kc.os.path.join(kc.CSRC, "kdtree_build.hip")).read()
    moved = src.replace("constexpr int kSmall = 256;", "constexpr int kSmall = 128;")
    assert moved != src
    k2 = kc.constants(moved, None)
    assert k2["kSmall"] == 128 and k2 != EXPECTED
    assert ("kSmall", [127, 128, 129]) in _missing_sizes(kc.SINGLE_SIZES, k2)
    k3 = kc.constants(src.replace("constexpr int kMid = 4096;", "constexpr int kMid = 8192;"), None)
    # (8 191..8 193 are in the list already; the edges of the chunked levels move out of it)
    assert k3["kHuge"] == 8192 and [b[1] for b in _missing_sizes(kc.SINGLE_SIZES, k3)] == [[16384], [32769]]


def test_the_mixed_set_is_the_one_the_gpu_test_describes():
    k = kc.constants()
    ns = [c[1] for c in kc.MIXED_SET]
    assert kc.chunked_levels(max(ns)) == 5
    # trees on both sides of every tier next to a tree that asks for five chunked levels
    assert {k["kMid"] + 1, k["kMid"], k["kSmall"] + 1, k["kSmall"], k["kLeafMax"] + 1, k["kLeafMax"], 1, 2 * k["kMid"] + 1} <= set(ns)
    assert [c[1] for c in kc.MANY_ROOTS] == list(range(1, 301)) and len(kc.MANY_ROOTS) > 256  # huge_root_kernel: 256 threads


def test_the_plan_round_case_has_more_than_256_chunked_tasks_in_its_last_level(dbg):
    """(d): huge_plan_block plans a level in rounds of 256 tasks.  One tree has at most 2^7 = 128 tasks at the last chunked level, so the
    second round needs a set: three balanced 600 000-point trees, 128 nodes each at depth 7 (of 4 530..4 927 points with these seeds)."""
    k = kc.constants()
    last = k["kHugeLevels"] - 1
    assert kc.chunked_levels(600000) == k["kHugeLevels"]
    cs = [kc.census(t) for t in kc.host_trees(dbg, kc.PLAN_ROUNDS_SET)]
    per_tree = [len(c["big"].get(last, ())) for c in cs]
    assert per_tree == [128, 128, 128] and sum(per_tree) > 256, per_tree
    sizes = np.concatenate([c["big"][last] for c in cs])
    print("sizes at depth %d: %d..%d" % (last, sizes.min(), sizes.max()))
    assert sizes.min() > k["kHuge"] and sizes.max() <= 2 * k["kHuge"], (sizes.min(), sizes.max())  # (all chunked; none left for a further level)
    want = kc.expected_stats(cs, 600000)
    assert want[kc.S_NTASKS + last] == 384 and want[kc.S_NCHUNKS + last] == 3 * 384 and want[kc.S_STRAGGLERS] == 0


def test_the_straggler_case_leaves_nodes_above_kmid_after_every_chunked_level(dbg):
    """(e): a balanced tree above 2^20 points -- 256 nodes at depth kHugeLevels (of 4 104..4 513 points with this seed) go to
    build_level_kernel."""
    k = kc.constants()
    L = k["kHugeLevels"]
    (variant, n, seed), = kc.STRAGGLER_SET
    assert kc.chunked_levels(n) == L and n > k["kMid"] << L
    c = kc.census(kc.host_tree(dbg, variant, n, seed))
    left = c["big"].get(L, np.zeros(0, np.int64))
    assert len(left) >= 1
    print("sizes at depth %d: %d..%d" % (L, left.min(), left.max()))
    assert len(left) == 256 and left.min() > k["kMid"], (len(left), left.min(), left.max())
    assert L + 1 not in c["big"]  # every one of them is finished in one split: 256 mid-queue pushes per half
    assert kc.expected_stats([c], n)[kc.S_STRAGGLERS] == 256


@pytest.mark.parametrize("n", kc.SINGLE_SIZES)
def test_host_builder_against_the_oracle_tree_at_every_tier_size(dbg, oracle, n):
    """The yardstick of the GPU file: the product's host builder gives the oracle's tree, node for node, at every size and variant of (a)."""
    for variant, m, seed in kc.single_cases():
        if m == n:
            p = kc.cloud(variant, n, seed)
            kc.assert_oracle_tree(kc.host_tree(dbg, variant, n, seed), p, oracle.kdtree_export(p))


@pytest.mark.parametrize("case", kc.PLAN_ROUNDS_SET + kc.STRAGGLER_SET, ids=lambda c: "%s-%d-%d" % c)
def test_host_builder_against_the_oracle_at_the_large_sizes(dbg, oracle, case):
    """(d) and (e): permutation and box only -- the permutation is the product of every split of the tree."""
    p = kc.cloud(*case)
    kc.assert_oracle_top(kc.host_tree(dbg, *case), p, oracle.kdtree_export(p))


def test_the_census_counts_what_the_walk_finds(dbg):
    """census() on trees small enough to count by hand."""
    k = kc.constants()
    one = kc.census(kc.host_tree(dbg, "uniform", 1, 38))
    assert one == dict(big={}, chunks={}, mid=0, small=1)
    c = kc.census(kc.host_tree(dbg, "identical", 257, 34))  # 257 identical points split 128 | 129: one mid root, two small children
    assert (c["big"], c["mid"], c["small"]) == ({}, 1, 2)
    c = kc.census(kc.host_tree(dbg, "identical", 8193, 40))  # 8 193 -> 4 096 | 4 097 -> 2 048 | 2 049
    assert {d: v.tolist() for d, v in c["big"].items()} == {0: [8193], 1: [4097]} and c["chunks"][0].tolist() == [5] and c["chunks"][1].tolist() == [3]
    # mid: 4 096, 2 048, 2 049.  small: halving 4 096 and 2 048 gives 16 + 8 nodes of 256; 2 049 -> 1 024 | 1 025 gives 4 + 2 + 1 of 256 and a
    # node of 257, whose two children are the last two
    assert c["mid"] == 3 and c["small"] == 16 + 8 + 7 + 2
    s = kc.expected_stats([c], 8193)
    assert s[kc.S_LEVELS] == 2 and s[kc.S_NTASKS:kc.S_NTASKS + 3].tolist() == [1, 1, 0] and s[kc.S_NCHUNKS:kc.S_NCHUNKS + 3].tolist() == [5, 3, 0]
    assert s[kc.S_STRAGGLERS] == 0 and k["kChunk"] == 2048
