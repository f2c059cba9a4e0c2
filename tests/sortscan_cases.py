"""Case lists and plain references for the three shared primitives: exclusive_scan_u32 and radix_sort_pairs_u32 / _u64 of csrc/sortscan.hip
and the fixed-order partial-sum reducer of csrc/reduce_partials.h, reached through the doors of the TEST-ONLY library (csrc/debug_hooks.h:
ps_debug_scan_* / ps_debug_sort_* / ps_debug_reduce_partials).  CPU only, numpy only: nothing here imports the package.

tests/test_sortscan_rule.py holds these lists to the regimes they claim (and the references to independent facts); tests/test_gpu_sortscan.py
parametrises over them."""
import ctypes

import numpy as np

# ---- the doors ---------------------------------------------------------------------------------------------------------------------------------


def bind(h):
    """Declares the argument types of the doors on a loaded libpointseg_debug.so handle and returns it."""
    c_vp, c_int, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    protos = {
        "ps_debug_scan_words": (i64, [i64]),
        "ps_debug_sort_words": (i64, [i64]),
        "ps_debug_scan_launches": (c_int, [i64]),
        "ps_debug_sort_launches": (c_int, [i64, c_int]),
        "ps_debug_scan_u32": (c_int, [c_vp, c_vp, c_vp, i64, c_vp]),
        "ps_debug_sort_pairs": (c_int, [c_vp, c_int, c_vp, c_vp, c_vp, c_vp, i64, c_int, c_vp, ctypes.POINTER(c_int)]),
        "ps_debug_reduce_partials": (c_int, [c_vp, c_int, c_vp, c_int, c_int, c_int, c_vp, c_vp]),
    }
    for name, (res, args) in protos.items():
        fn = getattr(h, name)
        fn.restype = res
        fn.argtypes = args
    return h


# ---- the scan ----------------------------------------------------------------------------------------------------------------------------------

SCAN_TILE = 2048  # kTile of sortscan.hip: elements per workgroup
SCAN_SIZES = [1, 7, 8, 9, 2047, 2048, 2049, 4097, 2048 * 2048 - 1, 2048 * 2048, 2048 * 2048 + 1, 5000011]
SCAN_PATTERNS = ["ones", "random", "tile_ends", "wrap"]
# (words `in` is moved off its 16-byte boundary, words `out` is, in place): the 16-byte path needs both aligned
SCAN_POINTERS = {"aligned": (0, 0, False), "in_place": (0, 0, True), "in_off": (1, 0, False), "out_off": (0, 1, False), "both_off": (1, 1, False)}
SCAN_CASES = [(n, pat, ptr) for n in SCAN_SIZES for pat in SCAN_PATTERNS for ptr in SCAN_POINTERS]


def scan_id(case):
    return "n%d-%s-%s" % case


def pad64(n):
    return (n + 63) // 64 * 64


def scan_levels(n):
    """Launch levels of exclusive_scan_u32: the tile kernel over n elements, over their totals, over the totals of those..."""
    levels, m = 1, -(-n // SCAN_TILE)
    while m > 1:
        levels, m = levels + 1, -(-m // SCAN_TILE)
    return levels


def scan_launches(n):
    """One tile launch per level and one add launch per level but the last."""
    return 0 if n == 0 else 2 * scan_levels(n) - 1


def scan_words(n):
    """64 + the padded tile counts of every level, the last level's single total included."""
    words, m = 64, -(-n // SCAN_TILE)
    while True:
        words += pad64(m)
        if m <= 1:
            return words
        m = -(-m // SCAN_TILE)


def scan_input(n, pattern):
    rng = np.random.default_rng(n % 1000003 + 17 * SCAN_PATTERNS.index(pattern))
    if pattern == "ones":  # out[i] == i
        return np.ones(n, np.uint32)
    if pattern == "random":
        return rng.integers(0, 4, n, dtype=np.uint32)
    if pattern == "tile_ends":  # sparse head flags, only on the last element of a tile: a tile's total comes from its last thread alone
        a = np.zeros(n, np.uint32)
        ends = np.arange(SCAN_TILE - 1, n, SCAN_TILE)
        a[ends[rng.random(len(ends)) < 0.5]] = 1
        if n >= SCAN_TILE:
            a[SCAN_TILE - 1] = 1
        return a
    assert pattern == "wrap"  # every value >= 2^31: the running total passes 2^32 at the third element and many times after
    return rng.integers(2 ** 31, 2 ** 32, n, dtype=np.uint32)


def scan_reference(a):
    """np.cumsum in uint64, shifted by one, mod 2^32."""
    out = np.zeros(len(a), np.uint64)
    np.cumsum(a[:-1], dtype=np.uint64, out=out[1:])
    return (out & np.uint64(0xFFFFFFFF)).astype(np.uint32)


# ---- the sort ----------------------------------------------------------------------------------------------------------------------------------

SORT_TILE = 8192  # kSortTile: keys per workgroup; a wave owns 2048 consecutive ones and walks them 64 at a time
SORT_SIZES = [1, 63, 64, 65, 2047, 2048, 2049, 8191, 8192, 8193, 8192 * 9 + 5, 300001]
SORT_BITS = {4: [1, 7, 8, 9, 16, 17, 24, 25, 32], 8: [1, 8, 9, 32, 33, 40, 41, 48, 49, 56, 57, 64]}
SORT_PATTERNS = ["uniform", "all_equal", "top_bit", "ascending", "descending", "runs_64", "runs_2048"]


def _sort_cases():
    """Not the full product: every width runs at the last single-tile size (8192), the first multi-tile size (8193), two sizes that rotate
    through the list and one of the two large ones; every (width, size) pair runs every pattern."""
    cases, j = [], 0
    for key_bytes, widths in SORT_BITS.items():
        for bits in widths:
            sizes = {SORT_SIZES[j % 12], SORT_SIZES[(j + 6) % 12], 8192, 8193, SORT_SIZES[10 + j % 2]}
            cases += [(key_bytes, n, bits, pat) for n in sorted(sizes) for pat in SORT_PATTERNS]
            j += 1
    return cases


SORT_CASES = _sort_cases()


def sort_id(case):
    return "u%d-n%d-b%d-%s" % (8 * case[0], case[1], case[2], case[3])


def sort_passes(bits):
    return 1 if bits <= 8 else -(-bits // 8)


def sort_which(bits):
    """The buffer pair that holds the result: the passes ping-pong from pair 0."""
    return sort_passes(bits) % 2


def sort_tiles(n):
    return -(-n // SORT_TILE)


def sort_launches(n, bits):
    """Per pass: the histogram, the scan of the 256 x tiles table, the scatter."""
    return 0 if n == 0 else sort_passes(bits) * (2 + scan_launches(256 * sort_tiles(n)))


def sort_words(n):
    table = pad64(256 * sort_tiles(n))
    return table + scan_words(table)


def sort_keys(key_bytes, n, bits, pattern):
    """uint32 / uint64 keys [n], no bit at or above `bits`."""
    dt = np.uint32 if key_bytes == 4 else np.uint64
    rng = np.random.default_rng(1000 * bits + n % 9973 + SORT_PATTERNS.index(pattern))
    top = (1 << bits) - 1  # the largest key

    def draw(m):
        return rng.integers(0, top, m, dtype=np.uint64, endpoint=True)

    if pattern == "uniform":
        k = draw(n)
    elif pattern == "all_equal":
        k = np.full(n, draw(1)[0], np.uint64)
    elif pattern == "top_bit":  # two values that differ only in the top bit: every pass but the last sees one digit
        low = int(draw(1)[0]) & (top >> 1)
        k = np.uint64(low) | (rng.integers(0, 2, n, dtype=np.uint64) << np.uint64(bits - 1))
    elif pattern in ("ascending", "descending"):  # non-decreasing over the whole key range (n may exceed 2^bits: equal neighbours)
        i = np.arange(n, dtype=np.uint64)
        k = i * np.uint64(min((1 << bits) // n, top)) if n <= 1 << bits else (i << np.uint64(bits)) // np.uint64(n)
        if pattern == "descending":
            k = k[::-1].copy()
    else:  # each aligned run of 64 (a round of one wave) / 2048 (a wave's whole span) keys equal
        run = 64 if pattern == "runs_64" else 2048
        k = draw(-(-n // run))[np.arange(n) // run]
    assert k.shape == (n,) and int(k.max()) <= top
    return k.astype(dt)


def sort_reference(keys):
    """(sorted keys, the stable permutation): with values arange(n) going in, the values coming out ARE the permutation."""
    order = np.argsort(keys, kind="stable")
    return keys[order], order.astype(np.uint32)


# ---- the reducer -------------------------------------------------------------------------------------------------------------------------------

REDUCE_FORMS = {0: (np.float32, np.float32), 1: (np.float64, np.float64), 2: (np.float32, np.float32), 3: (np.float32, np.float64)}  # form: (T, A)
REDUCE_N_PART = [1, 15, 16, 17, 32, 33, 48, 49, 63, 64, 65, 112, 113, 129, 800, 3000]
REDUCE_NV = [1, 15, 16, 17, 72, 100]
REDUCE_CASES = [(form, n_part, nv) for form in REDUCE_FORMS for n_part in REDUCE_N_PART for nv in REDUCE_NV]
# a1 / a2 / a3 are first used at 17 / 33 / 49 partials, where the unrolled loop also first runs; it runs a second time at 113
REDUCE_THRESHOLDS = [17, 33, 49, 113]


def reduce_id(case):
    return "form%d-p%d-v%d" % case


def reduce_n0s(nv):
    """The splits of forms 2 and 3: nothing / everything in out0, 64 of 72 (convbn_rows.hip's weights and bias), and one that is no multiple of 16."""
    odd = nv // 2 if (nv // 2) % 16 else nv // 2 + 1
    return sorted({0, nv, min(odd, nv)} | ({64} if nv == 72 else set()))


def reducer_regimes(n_part):
    """(the set of loop-iteration counts, the set of tail patterns) over the 16 groups; a tail pattern = which of a0 / a1 / a2 take one more
    partial after the loop."""
    iters, tails = set(), set()
    for g in range(16):
        b, it = g, 0
        while b + 48 < n_part:
            b, it = b + 64, it + 1
        iters.add(it)
        tails.add((b < n_part, b + 16 < n_part, b + 32 < n_part))
    return iters, tails


def reduce_input(form, n_part, nv, kind):
    """kind "integer": random integers of magnitude <= 2^10 (no float32 sum of 3000 of them rounds: exact in every order); "normal"."""
    rng = np.random.default_rng(100000 * form + 100 * n_part + nv + (0 if kind == "integer" else 7))
    if kind == "integer":
        return rng.integers(-1024, 1024, (n_part, nv), endpoint=True).astype(REDUCE_FORMS[form][0])
    return (rng.standard_normal((n_part, nv)) * 10.0 ** rng.uniform(-2, 2, (n_part, 1))).astype(REDUCE_FORMS[form][0])


def reduce_reference(part, form):
    """The kernel's ONE fixed order, restated: per group g the four chains over b = g, g + 16, ... as the loop and the tails deal them, then
    (a0 + a1) + (a2 + a3), then the four-by-four tree over the groups; every add in the form's accumulator type, the result in its value type."""
    T, A = REDUCE_FORMS[form]
    n_part, nv = part.shape
    assert part.dtype == T
    red = []
    for g in range(16):
        a = [np.zeros(nv, A) for _ in range(4)]
        b = g
        while b + 48 < n_part:
            for j in range(4):
                a[j] = a[j] + part[b + 16 * j].astype(A)
            b += 64
        for j in range(3):
            if b + 16 * j < n_part:
                a[j] = a[j] + part[b + 16 * j].astype(A)
        red.append((a[0] + a[1]) + (a[2] + a[3]))
    s = np.zeros(nv, A)
    for k in range(0, 16, 4):
        s = s + ((red[k] + red[k + 1]) + (red[k + 2] + red[k + 3]))
    assert s.dtype == A
    return s.astype(T)


def reduce_exact(part):
    """The exact sum of integer-valued partials."""
    assert np.array_equal(part, np.rint(part))
    return part.astype(np.int64).sum(0)


# ---- what the lists must reach (tests/test_sortscan_rule.py) ----------------------------------------------------------------------------------

def scan_gaps(sizes):
    """What a list of scan sizes misses: 1, 2 and 3 levels, the last size of a level and the first of the next."""
    want = [("levels %d" % l, lambda n, l=l: scan_levels(n) == l) for l in (1, 2, 3)]
    want += [("n = %d" % n, lambda m, n=n: m == n) for t in (SCAN_TILE, SCAN_TILE ** 2) for n in (t, t + 1)]
    want += [("a ragged size of 3 levels", lambda n: scan_levels(n) == 3 and n % SCAN_TILE not in (0, 1, SCAN_TILE - 1)),
             ("one thread's 8 words", lambda n: n == 8), ("below 8 words", lambda n: n < 8), ("8 words and a tail", lambda n: n == 9)]
    return [name for name, ok in want if not any(ok(n) for n in sizes)]


def sort_gaps(cases):
    """What a list of sort cases misses: every size and width of the lists, every pass count of a key width's list (1-8 between
    them) on a single tile and on several and with every pattern, a two-level table scan."""
    miss = ["size %d" % n for n in SORT_SIZES if not any(c[1] == n for c in cases)]
    for kb, widths in SORT_BITS.items():
        miss += ["u%d width %d" % (8 * kb, b) for b in widths if not any(c[0] == kb and c[2] == b for c in cases)]
        for p in sorted({sort_passes(b) for b in widths}):
            mine = [c for c in cases if c[0] == kb and sort_passes(c[2]) == p]
            if not any(sort_tiles(c[1]) == 1 for c in mine):
                miss.append("u%d %d passes on one tile" % (8 * kb, p))
            if not any(sort_tiles(c[1]) > 1 for c in mine):
                miss.append("u%d %d passes on several tiles" % (8 * kb, p))
            miss += ["u%d %d passes %s" % (8 * kb, p, pat) for pat in SORT_PATTERNS if not any(c[3] == pat for c in mine)]
    miss += ["%d passes" % p for p in range(1, 9) if not any(sort_passes(c[2]) == p for c in cases)]
    if not any(scan_levels(256 * sort_tiles(c[1])) == 2 for c in cases):
        miss.append("a two-level table scan")
    return miss


def reduce_gaps(n_parts):
    """What a list of partial counts misses: both sides of every threshold, the iteration-count sets {0}, {0, 1}, {1}, {1, 2} and a higher
    one, and every tail pattern that exists at all (a sweep over 1..200)."""
    miss = ["n_part %d" % n for t in REDUCE_THRESHOLDS for n in (t - 1, t) if n not in n_parts]
    have = [reducer_regimes(n) for n in n_parts]
    miss += ["iterations %s" % sorted(s) for s in ({0}, {0, 1}, {1}, {1, 2}) if not any(h[0] == s for h in have)]
    if not any(max(h[0]) > 2 for h in have):
        miss.append("iterations above 2")
    every_tail = set().union(*(reducer_regimes(n)[1] for n in range(1, 201)))
    # a mixed tail: some groups done, others with one to three partials left
    every_mix = {frozenset(reducer_regimes(n)[1]) for n in range(1, 201)}
    miss += ["tail %s" % (t,) for t in sorted(every_tail - set().union(*(h[1] for h in have)))]
    miss += ["tail mix %s" % sorted(m) for m in sorted(every_mix - {frozenset(h[1]) for h in have}, key=sorted)]
    return miss
