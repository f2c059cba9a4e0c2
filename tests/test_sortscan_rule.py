"""CPU tests behind tests/test_gpu_sortscan.py: the plain references of tests/sortscan_cases.py against independent facts, the case lists
against the regimes they claim to reach (a list cut below a regime must fail), and the host-only doors of the debug library
(ps_debug_scan_words / _sort_words / _scan_launches / _sort_launches: the product's own sizing functions) against closed forms restated in
Python -- the callers carve these regions out of shared arenas, so an under-count would write into a neighbour's memory."""
import ast
import math
import os

import numpy as np
import pytest

import sortscan_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GPU_MODULE = os.path.join(ROOT, "tests", "test_gpu_sortscan.py")
# the GPU tests and the list of sortscan_cases each must be parametrised over
GPU_LISTS = {"test_exclusive_scan": "SCAN_CASES", "test_radix_sort_pairs": "SORT_CASES", "test_reduce_partials": "REDUCE_CASES"}


# ---- the references against independent facts -------------------------------------------------------------------------------------------------

def test_scan_reference_on_small_cases():
    assert cases.scan_reference(np.array([5], np.uint32)).tolist() == [0]
    assert cases.scan_reference(np.array([3, 0, 2, 1], np.uint32)).tolist() == [0, 3, 3, 5]
    big = np.array([0xFFFFFFFF, 2, 0x80000000, 0x80000000, 1], np.uint32)
    assert cases.scan_reference(big).tolist() == [0, 0xFFFFFFFF, 1, 0x80000001, 1]
    for n in (1, 2, 9, 2049):
        for pat in cases.SCAN_PATTERNS:
            a = cases.scan_input(n, pat)
            want, run = [], 0
            for x in a.tolist():
                want.append(run)
                run = (run + x) % 2 ** 32
            assert a.dtype == np.uint32 and cases.scan_reference(a).tolist() == want
    assert np.array_equal(cases.scan_reference(cases.scan_input(4097, "ones")), np.arange(4097))
    ends = cases.scan_input(5000, "tile_ends")
    assert ends.sum() >= 1 and not np.delete(ends, [2047, 4095]).any()
    wrap = cases.scan_input(3, "wrap")
    assert int(wrap.astype(np.uint64).sum()) > 2 ** 32


def test_sort_reference_against_sorted_with_an_index_tiebreak():
    for key_bytes, n, bits, pat in [(4, 300, 3, "uniform"), (8, 257, 41, "top_bit"), (8, 200, 64, "runs_64"), (4, 100, 6, "descending")]:
        keys = cases.sort_keys(key_bytes, n, bits, pat)
        want = sorted(range(n), key=lambda i: (int(keys[i]), i))
        got_keys, got_order = cases.sort_reference(keys)
        assert got_order.tolist() == want and got_keys.tolist() == [int(keys[i]) for i in want]
        assert len(set(keys.tolist())) < n  # equal keys: the tiebreak decides something


def test_sort_keys_stay_below_their_width_and_have_their_shape():
    for key_bytes, widths in cases.SORT_BITS.items():
        for bits in widths:
            for pat in cases.SORT_PATTERNS:
                for n in (1, 65, 8193):
                    k = cases.sort_keys(key_bytes, n, bits, pat)
                    assert k.dtype == (np.uint32 if key_bytes == 4 else np.uint64) and k.shape == (n,) and not (k.astype(object) >> bits).any()
    k = cases.sort_keys(8, 8193, 57, "top_bit")
    assert len(set(k.tolist())) == 2 and len(set((k ^ k[0]).tolist()) - {0, 1 << 56}) == 0
    assert len(set(cases.sort_keys(8, 8193, 57, "all_equal").tolist())) == 1
    asc, desc = cases.sort_keys(8, 8193, 64, "ascending"), cases.sort_keys(8, 8193, 64, "descending")
    assert (np.diff(asc.astype(object)) > 0).all() and (np.diff(desc.astype(object)) < 0).all()
    assert (np.diff(cases.sort_keys(4, 8193, 7, "ascending").astype(np.int64)) >= 0).all()
    for pat, run in (("runs_64", 64), ("runs_2048", 2048)):
        k = cases.sort_keys(8, 8193, 49, pat)
        starts = np.flatnonzero(np.diff(k.astype(object)) != 0) + 1
        assert len(starts) == 8192 // run and not (starts % run).any()


def test_reducer_reference_is_exact_on_integers():
    for form in cases.REDUCE_FORMS:
        for n_part in (1, 17, 49, 113, 3000):
            part = cases.reduce_input(form, n_part, 17, "integer")
            assert np.abs(part).max() <= 1024 and part.dtype == cases.REDUCE_FORMS[form][0]
            got = cases.reduce_reference(part, form)
            assert got.dtype == part.dtype and np.array_equal(got.astype(np.int64), cases.reduce_exact(part))


def test_reducer_reference_is_close_to_fsum_on_normal_data():
    for form, (T, A) in cases.REDUCE_FORMS.items():
        for n_part in (15, 49, 113, 800):
            part = cases.reduce_input(form, n_part, 16, "normal")
            got = cases.reduce_reference(part, form)
            for i in range(16):
                col = [float(x) for x in part[:, i]]
                bound = n_part * float(np.finfo(A).eps) * math.fsum(abs(x) for x in col)
                if A != T:  # the final cast of the float64 sum to float32
                    bound += float(np.finfo(T).eps) * abs(math.fsum(col))
                assert abs(float(got[i]) - math.fsum(col)) <= bound
    # and the order matters at all: float32 sums in plain order give other bytes
    part = cases.reduce_input(0, 800, 16, "normal")
    plain = np.zeros(16, np.float32)
    for row in part:
        plain = plain + row
    assert not np.array_equal(plain, cases.reduce_reference(part, 0))


# ---- the lists reach what they claim -----------------------------------------------------------------------------------------------------------

def test_scan_sizes_reach_every_level_on_both_sides_of_each_threshold():
    assert cases.scan_gaps(cases.SCAN_SIZES) == []
    assert [cases.scan_levels(n) for n in (1, 2048, 2049, 2048 ** 2, 2048 ** 2 + 1, 5000011)] == [1, 1, 2, 2, 3, 3]
    assert set(cases.SCAN_CASES) == {(n, p, q) for n in cases.SCAN_SIZES for p in cases.SCAN_PATTERNS for q in cases.SCAN_POINTERS}
    assert max(cases.SCAN_SIZES) < 5.1e6
    ptr = cases.SCAN_POINTERS
    assert {(i % 4 != 0, o % 4 != 0, same) for i, o, same in ptr.values()} == {(False, False, False), (False, False, True), (True, False, False),
                                                                                 (False, True, False), (True, True, False)}


def test_sort_cases_reach_every_size_width_and_pass_count():
    assert cases.sort_gaps(cases.SORT_CASES) == []
    assert {cases.sort_passes(b) for b in cases.SORT_BITS[4]} == {1, 2, 3, 4} and {cases.sort_passes(b) for b in cases.SORT_BITS[8]} == {1, 2, 4, 5, 6, 7, 8}
    assert [cases.sort_passes(b) for b in (1, 8, 9, 16, 17, 40, 41, 56, 57, 64)] == [1, 1, 2, 2, 3, 5, 6, 7, 8, 8]
    assert [cases.sort_which(b) for b in (8, 9, 24, 32, 41, 57)] == [1, 0, 1, 0, 0, 0] and cases.sort_which(33) == 1
    assert cases.scan_levels(256 * cases.sort_tiles(8192 * 9 + 5)) == 2 and cases.scan_levels(256 * cases.sort_tiles(8192 * 8)) == 1
    assert len(cases.SORT_CASES) == len(set(cases.SORT_CASES)) and max(c[1] for c in cases.SORT_CASES) <= 300001
    assert all(c[2] <= 8 * c[0] for c in cases.SORT_CASES)


def test_reducer_counts_reach_every_regime():
    assert cases.reduce_gaps(cases.REDUCE_N_PART) == []
    r = cases.reducer_regimes
    assert [r(n)[0] for n in (48, 49, 64, 112, 113, 129, 800, 3000)] == [{0}, {0, 1}, {1}, {1}, {1, 2}, {2}, {12}, {46, 47}]
    assert r(1)[1] == {(False, False, False), (True, False, False)} and r(16)[1] == {(True, False, False)}
    assert r(17)[1] == {(True, False, False), (True, True, False)} and r(33)[1] == {(True, True, False), (True, True, True)}
    assert r(49)[1] == {(False, False, False), (True, True, True)}  # group 0 went through the loop and has nothing left
    assert set(cases.REDUCE_CASES) == {(f, p, v) for f in range(4) for p in cases.REDUCE_N_PART for v in cases.REDUCE_NV}
    assert [cases.reduce_n0s(nv) for nv in (1, 16, 72, 100)] == [[0, 1], [0, 8, 16], [0, 36, 64, 72], [0, 50, 100]]
    assert all(any(n0 % 16 for n0 in cases.reduce_n0s(nv)) for nv in cases.REDUCE_NV)


def test_the_guards_see_a_cut_list():
    """In memory: a size, a width or a partial count that carries a regime is removed, and the check above would fail."""
    for n, what in ((2048, "n = 2048"), (2049, "n = 2049"), (2048 ** 2 + 1, "n = 4194305"), (8, "one thread's 8 words")):
        assert cases.scan_gaps([m for m in cases.SCAN_SIZES if m != n]) == [what]
    assert cases.scan_gaps([n for n in cases.SCAN_SIZES if n <= 2048 ** 2]) == ["levels 3", "n = 4194305", "a ragged size of 3 levels"]
    assert cases.scan_gaps([n for n in cases.SCAN_SIZES if n != 5000011]) == ["a ragged size of 3 levels"]

    cut = lambda keep: cases.sort_gaps([c for c in cases.SORT_CASES if keep(c)])
    assert cut(lambda c: c[1] != 8191) == ["size 8191"]
    assert cut(lambda c: (c[0], c[2]) != (8, 41)) == ["u64 width 41"]  # 48 still gives six passes
    assert set(cut(lambda c: not (c[0] == 8 and c[2] in (41, 48)))) >= {"u64 width 41", "u64 width 48", "u64 6 passes on one tile",
                                                                         "u64 6 passes on several tiles", "u64 6 passes uniform"}
    assert cut(lambda c: not (c[0] == 8 and c[2] > 56 and c[1] > 8192)) == ["u64 8 passes on several tiles"]
    assert cut(lambda c: not (c[0] == 4 and c[2] > 24 and c[1] <= 8192)) == ["u32 4 passes on one tile"]
    assert cut(lambda c: not (c[3] == "runs_2048" and 40 < c[2] <= 48)) == ["u64 6 passes runs_2048"]
    assert "a two-level table scan" in cut(lambda c: c[1] < 8192 * 9)

    for n in (16, 17, 32, 33, 48, 49, 112, 113):
        assert "n_part %d" % n in cases.reduce_gaps([m for m in cases.REDUCE_N_PART if m != n])
    assert "iterations [1, 2]" in cases.reduce_gaps([m for m in cases.REDUCE_N_PART if m != 113])
    assert "iterations above 2" in cases.reduce_gaps([m for m in cases.REDUCE_N_PART if m < 800])
    assert any(g.startswith("tail") for g in cases.reduce_gaps([m for m in cases.REDUCE_N_PART if m not in (17, 32)]))


# ---- the GPU module runs these lists -----------------------------------------------------------------------------------------------------------

def _parametrize_sources(src):
    """{test name: [the source text of the list of each of its parametrize marks]}."""
    out = {}
    for node in ast.parse(src).body:
        if isinstance(node, ast.FunctionDef) and node.name.startswith("test_"):
            out[node.name] = [ast.unparse(d.args[1]) for d in node.decorator_list
                              if isinstance(d, ast.Call) and getattr(d.func, "attr", "") == "parametrize"]
    return out


def _foreign_lists(src):
    """The GPU tests that are not parametrised over exactly their list of sortscan_cases (imported as `cases`)."""
    got = _parametrize_sources(src)
    return sorted(name for name, lst in GPU_LISTS.items() if got.get(name) != ["cases." + lst])


def test_the_gpu_module_is_parametrised_over_these_lists():
    src = open(GPU_MODULE).read()
    assert "import sortscan_cases as cases\n" in src and _foreign_lists(src) == []
    # in memory: a literal list of its own, and a slice of the shared one
    own = src.replace('cases.SCAN_CASES', '[(8, "ones", "aligned")]', 1)
    assert own != src and _foreign_lists(own) == ["test_exclusive_scan"]
    short = src.replace("cases.SORT_CASES", "cases.SORT_CASES[:10]", 1)
    assert short != src and _foreign_lists(short) == ["test_radix_sort_pairs"]
    gone = src.replace("def test_reduce_partials(", "def test_reduce_partials_off(")
    assert gone != src and _foreign_lists(gone) == ["test_reduce_partials"]


# ---- the host-only doors -----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def doors(lib):
    import ctypes
    return cases.bind(ctypes.CDLL(os.path.join(ROOT, "point-unet_amd", "libpointseg_debug.so")))


def test_scan_workspace_and_launches_against_the_closed_forms(doors):
    sizes = sorted(set(cases.SCAN_SIZES) | set(cases.SORT_SIZES) | {256 * cases.sort_tiles(n) for n in cases.SORT_SIZES} | {0, 2048 ** 3, 2048 ** 3 + 1})
    for n in sizes:
        assert doors.ps_debug_scan_words(n) == cases.scan_words(n), n
        assert doors.ps_debug_scan_launches(n) == cases.scan_launches(n), n
    # the closed form itself, by hand: 64 + pad64 of the tile counts per level
    assert cases.scan_words(1) == 64 + 64 and cases.scan_words(2049) == 64 + 64 + 64 and cases.scan_words(2048 ** 2 + 1) == 64 + 2112 + 64 + 64
    assert [cases.scan_launches(n) for n in (0, 1, 2048, 2049, 2048 ** 2, 2048 ** 2 + 1)] == [0, 1, 1, 3, 3, 5]
    assert doors.ps_debug_scan_words(-1) == -1 and doors.ps_debug_scan_launches(-1) == -1


def test_the_scan_workspace_holds_every_level(doors):
    """What exclusive_scan_u32 touches, walked level by level: level l writes one total per tile at its `work` and hands work + pad64(tiles) on."""
    for n in cases.SCAN_SIZES + [256 * cases.sort_tiles(n) for n in cases.SORT_SIZES]:
        off, m = 0, n
        while True:
            tiles = -(-m // cases.SCAN_TILE)
            end = off + tiles  # sums[0 .. tiles)
            if tiles <= 1:
                break
            off, m = off + cases.pad64(tiles), tiles
        assert end <= doors.ps_debug_scan_words(n), n


def test_sort_workspace_and_launches_against_the_closed_forms(doors):
    for n in cases.SORT_SIZES + [0, 8192 * 8, 8192 * 8 + 1]:
        assert doors.ps_debug_sort_words(n) == cases.sort_words(n), n
        table = cases.pad64(256 * cases.sort_tiles(n))
        assert 256 * cases.sort_tiles(n) + cases.scan_words(256 * cases.sort_tiles(n)) <= doors.ps_debug_sort_words(n)
        assert table % 64 == 0
        for widths in cases.SORT_BITS.values():
            for bits in widths:
                assert doors.ps_debug_sort_launches(n, bits) == cases.sort_launches(n, bits), (n, bits)
    assert cases.sort_words(1) == 256 + 64 + 64 and cases.sort_words(8193) == 512 + 64 + 64 and cases.sort_words(8192 * 9 + 5) == 2560 + 64 + 64 + 64
    assert cases.sort_launches(1, 64) == 8 * 3 and cases.sort_launches(8192 * 9 + 5, 33) == 5 * 5 and cases.sort_launches(8192 * 8, 9) == 2 * 3
    assert doors.ps_debug_sort_words(-1) == -1 and doors.ps_debug_sort_launches(-1, 8) == -1
    assert doors.ps_debug_sort_launches(10, 0) == -1 and doors.ps_debug_sort_launches(10, 65) == -1


def test_the_device_doors_refuse_bad_arguments_before_any_launch(doors, lib):
    """NULL pointers, negative sizes, a key width that is neither 4 nor 8: PS_EINVAL (1) on a machine without a GPU -- nothing was launched.  The
    non-NULL arguments are host addresses no kernel ever sees."""
    import ctypes
    buf = (ctypes.c_uint32 * 16)()
    p, which = ctypes.addressof(buf), ctypes.c_int(7)
    assert doors.ps_debug_scan_u32(None, p, p, 4, p) == 1
    assert doors.ps_debug_scan_u32(p, None, p, 4, p) == 1 and doors.ps_debug_scan_u32(p, p, None, 4, p) == 1
    assert doors.ps_debug_scan_u32(p, p, p, 4, None) == 1 and doors.ps_debug_scan_u32(p, p, p, -1, p) == 1
    ok = [p, 8, p, p, p, p, 4, 33, p, ctypes.byref(which)]
    for i, bad in ((0, None), (1, 2), (1, 16), (2, None), (3, None), (4, None), (5, None), (6, -1), (7, 0), (7, 65), (8, None), (9, None)):
        args = list(ok)
        args[i] = bad
        assert doors.ps_debug_sort_pairs(*args) == 1, i
    assert doors.ps_debug_sort_pairs(p, 4, p, p, p, p, 4, 33, p, ctypes.byref(which)) == 1  # 33 bits in a 32-bit key
    assert which.value == 7
    ok = [p, 3, p, 4, 16, 8, p, p]
    for i, bad in ((0, None), (1, -1), (1, 4), (2, None), (3, -1), (4, -1), (5, -1), (5, 17), (6, None), (7, None)):
        args = list(ok)
        args[i] = bad
        assert doors.ps_debug_reduce_partials(*args) == 1, i
    assert doors.ps_debug_reduce_partials(p, 0, p, 4, 16, 0, None, None) == 1
    assert b"ps_debug_reduce_partials" in lib.ps_last_error()
