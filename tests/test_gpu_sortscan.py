"""The shared scan, radix sort (csrc/sortscan.hip) and partial-sum reducer (csrc/reduce_partials.h) on their own, through the doors of the
TEST-ONLY library (csrc/debug_hooks.h), against the plain references of tests/sortscan_cases.py: the scan against np.cumsum in uint64, the
sort against numpy's stable argsort (values arange(n): the permutation itself is compared, so stability is), the reducer byte for byte
against its one fixed order restated in numpy and, on integer partials, against the exact sum.

Every device array -- inputs, results and the workspace of exactly the reported size -- lies between two guard bands of 4096 sentinel words
in its own allocation; all bands are checked after every call.  Every call runs twice and must give the same bytes.  The case lists are
sortscan_cases': tests/test_sortscan_rule.py holds them to the regimes they must reach (scan levels and the 16-byte / scalar paths, sort
pass counts 1-8 on one and on several tiles, the reducer's loop counts and tails) and this module to those lists."""
import ctypes
import functools
import os

import numpy as np
import pytest

import sortscan_cases as cases

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAND = 4096 * 4  # bytes: 4096 sentinel words


@pytest.fixture(scope="module")
def doors(lib):
    return cases.bind(ctypes.CDLL(os.path.join(ROOT, "point-unet_amd", "libpointseg_debug.so")))


def _ctx():
    from point_unet_amd import runtime
    ctx = runtime.default_context(0)
    ctx.use_torch_stream()
    return ctx.handle


def _check(rc):
    from point_unet_amd import _lib
    _lib.check(rc)


class Banded:
    """nbytes of device memory between two bands of 0xA5 bytes in one allocation; shift: bytes the array starts past its 16-byte boundary
    (they belong to the band in front)."""

    def __init__(self, nbytes, shift=0):
        self.lo, self.hi = BAND + shift, BAND + shift + nbytes
        self.buf = torch.full((self.hi + BAND,), 0xA5, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.ptr = ctypes.c_void_p(self.buf.data_ptr() + self.lo)  # (not a view's data_ptr: an empty view has none)

    def put(self, a):
        self.buf[self.lo:self.hi].copy_(torch.from_numpy(a.reshape(-1).view(np.uint8)))
        return self

    def get(self, dtype):
        return self.buf[self.lo:self.hi].cpu().numpy().view(dtype)

    def intact(self):
        return bool((self.buf[:self.lo] == 0xA5).all()) and bool((self.buf[self.hi:] == 0xA5).all())


def _intact(*arrays):
    for i, a in enumerate(arrays):
        assert a.intact(), "a guard band of array %d was written" % i


# ---- the scan ----------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=2)  # (the cases of one (size, pattern) are neighbours in the list: the reference is computed once for them)
def _scan_data(n, pattern):
    a = cases.scan_input(n, pattern)
    return a, cases.scan_reference(a)


@pytest.mark.parametrize("case", cases.SCAN_CASES, ids=cases.scan_id)
def test_exclusive_scan(doors, case):
    n, pattern, pointers = case
    in_off, out_off, in_place = cases.SCAN_POINTERS[pointers]
    a, want = _scan_data(n, pattern)
    work = Banded(4 * doors.ps_debug_scan_words(n))
    src = Banded(4 * n, 4 * in_off).put(a)
    dst = src if in_place else Banded(4 * n, 4 * out_off)
    assert src.ptr.value % 16 == 4 * in_off and dst.ptr.value % 16 == 4 * out_off
    ctx, runs = _ctx(), []
    for _ in range(2):  # (the second run finds the first one's totals in the workspace: nothing may depend on what it holds)
        if in_place:
            src.put(a)
        _check(doors.ps_debug_scan_u32(ctx, src.ptr, dst.ptr, n, work.ptr))
        runs.append(dst.get(np.uint32))
        _intact(work, src, dst)
    assert np.array_equal(runs[0], want)
    assert runs[0].tobytes() == runs[1].tobytes()
    assert in_place or np.array_equal(src.get(np.uint32), a)


# ---- the sort ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", cases.SORT_CASES, ids=cases.sort_id)
def test_radix_sort_pairs(doors, case):
    key_bytes, n, bits, pattern = case
    keys = cases.sort_keys(key_bytes, n, bits, pattern)
    want_keys, want_values = cases.sort_reference(keys)
    values = np.arange(n, dtype=np.uint32)
    work = Banded(4 * doors.ps_debug_sort_words(n))
    k, v = [Banded(key_bytes * n), Banded(key_bytes * n)], [Banded(4 * n), Banded(4 * n)]
    ctx, runs = _ctx(), []
    for _ in range(2):
        k[0].put(keys)  # (pair 0 is the input and, from two passes on, a ping-pong buffer)
        v[0].put(values)
        which = ctypes.c_int(-1)
        _check(doors.ps_debug_sort_pairs(ctx, key_bytes, k[0].ptr, k[1].ptr, v[0].ptr, v[1].ptr, n, bits, work.ptr, ctypes.byref(which)))
        assert which.value == cases.sort_which(bits)
        runs.append((k[which.value].get(keys.dtype), v[which.value].get(np.uint32)))
        _intact(work, *k, *v)
    assert np.array_equal(runs[0][1], want_values)  # the stable permutation
    assert np.array_equal(runs[0][0], want_keys)
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes()


# ---- the reducer -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", cases.REDUCE_CASES, ids=cases.reduce_id)
def test_reduce_partials(doors, case):
    form, n_part, nv = case
    T = cases.REDUCE_FORMS[form][0]
    size = np.dtype(T).itemsize
    ctx = _ctx()
    for kind in ("integer", "normal"):
        part = cases.reduce_input(form, n_part, nv, kind)
        want = cases.reduce_reference(part, form)
        src = Banded(size * n_part * nv).put(part)
        for n0 in cases.reduce_n0s(nv) if form >= 2 else [nv]:
            out0, out1 = Banded(size * n0), Banded(size * (nv - n0))
            runs = []
            for _ in range(2):
                _check(doors.ps_debug_reduce_partials(ctx, form, src.ptr, n_part, nv, n0, out0.ptr, out1.ptr if form >= 2 else None))
                runs.append(np.concatenate([out0.get(T), out1.get(T)]))
                _intact(src, out0, out1)
            what = "%s partials, n0 = %d" % (kind, n0)
            assert runs[0].tobytes() == want.tobytes(), what  # the ONE fixed order, byte for byte
            assert runs[0].tobytes() == runs[1].tobytes(), what
            if kind == "integer":  # exact in every order: a dropped or doubled partial has no tolerance to hide behind
                assert np.array_equal(runs[0].astype(np.int64), cases.reduce_exact(part)), what
        assert np.array_equal(src.get(T), part.reshape(-1))
