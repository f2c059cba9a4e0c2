"""The K-NN search is compiled per list size K: PS_KNN_KS in csrc/kdtree.h is the one list behind knn_kernel<K>, knn_pair_kernel<K> and
the host door ps_debug_knn_host.  These CPU tests hold the per-K tests to that list -- tests/test_gpu_knn_sizes.py on the kernels,
tests/test_host_logic.py on the host door: a size added to the header without a test fails here, and so does a size dropped from a
test's list."""
import ast
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the tests that must run at every compiled K: file -> names
PER_K_TESTS = {
    "test_gpu_knn_sizes.py": ["test_plain_kernel_self_queries", "test_plain_kernel_queries_outside_the_support", "test_plain_kernel_tiny_clouds",
                              "test_pyramid_at_the_seed_thresholds", "test_pyramid_of_two_clouds"],
    "test_host_logic.py": ["test_search_routine_matches_oracle_at_every_compiled_k"],
}


def _header_sizes(src=None):
    """The sizes of PS_KNN_KS in the default build (the #else branch of PS_KNN_FEW_K), in order."""
    if src is None:
        src = open(os.path.join(ROOT, "point-unet_amd", "csrc", "kdtree.h")).read()
    pair = re.search(r"#ifdef PS_KNN_FEW_K\n#define PS_KNN_PAIR_KS\(X\)[^\n]*\n#else\n#define PS_KNN_PAIR_KS\(X\)([^\n]*)\n#endif", src)
    assert pair, "PS_KNN_PAIR_KS not found in kdtree.h"
    all_ks = re.search(r"#define PS_KNN_KS\(X\)([^\n]*)\n", src).group(1)
    assert re.fullmatch(r"(\s*X\(\d+\))*\s*PS_KNN_PAIR_KS\(X\)\s*", all_ks), all_ks
    own = [int(k) for k in re.findall(r"X\((\d+)\)", all_ks)]
    body = pair.group(1)
    assert re.fullmatch(r"(\s*X\(\d+\))+\s*", body), body
    return own + [int(k) for k in re.findall(r"X\((\d+)\)", body)]


def _k_lists(src):
    """{test name: the K list of its @pytest.mark.parametrize("K", ...)} of one test source; a list given by name is looked up among
    the module's own literal assignments."""
    tree = ast.parse(src)
    consts = {}
    for node in tree.body:
        if isinstance(node, ast.Assign) and len(node.targets) == 1 and isinstance(node.targets[0], ast.Name):
            try:
                consts[node.targets[0].id] = ast.literal_eval(node.value)
            except ValueError:
                pass
    out = {}
    for node in tree.body:
        if not isinstance(node, ast.FunctionDef):
            continue
        for dec in node.decorator_list:
            if isinstance(dec, ast.Call) and getattr(dec.func, "attr", "") == "parametrize" and isinstance(dec.args[0], ast.Constant) and dec.args[0].value == "K":
                arg = dec.args[1]
                out[node.name] = list(consts[arg.id] if isinstance(arg, ast.Name) else ast.literal_eval(arg))
    return out


def _untested(sizes, sources):
    """[(file, test, sizes of the header the test does not run, sizes it runs that are not compiled)]; empty = in step."""
    bad = []
    for f, names in PER_K_TESTS.items():
        lists = _k_lists(sources[f])
        for name in names:
            got = lists.get(name, [])
            if sorted(got) != sorted(sizes) or len(got) != len(set(got)):
                bad.append((f, name, sorted(set(sizes) - set(got)), sorted(set(got) - set(sizes))))
    return bad


def _sources():
    return {f: open(os.path.join(ROOT, "tests", f)).read() for f in PER_K_TESTS}


def test_the_header_list_parses():
    sizes = _header_sizes()
    assert sizes[0] == 1 and sizes == sorted(set(sizes)) and {2, 3, 16, 32, 48, 64} <= set(sizes) and len(sizes) >= 21


def test_every_compiled_k_is_run_by_the_gpu_and_the_host_tests():
    assert _untested(_header_sizes(), _sources()) == []


def test_the_refused_sizes_are_not_compiled():
    import test_gpu_knn_sizes as t
    assert not set(t.REFUSED_KS) & set(_header_sizes())
    # one K of each store path, and the long lists
    assert [k % 4 == 0 for k in t.STORE_PATH_KS] == [False, True] and set(t.STORE_PATH_KS + t.DEEP_STACK_KS) <= set(_header_sizes())


def test_the_pyramid_sizes_reach_every_seed_form_of_every_k():
    """Both levels of test_pyramid_at_the_seed_thresholds' clouds, by the rule of knn_body: every K > 1 starts from the single K window,
    every K <= 32 also from the 2K-1 window, and a level below K points runs unseeded (K = 2 cannot: a level of one point would leave
    the level under it empty).  Each form is met on both sides of its threshold."""
    import test_gpu_knn_sizes as t
    for K in _header_sizes():
        levels = {n for n0 in t.pyramid_sizes(K) for n in (n0, n0 // 2)}
        forms = {t.seed_form(K, nq) for nq in levels}
        want = {"unseeded"} if K == 1 else {"single_window"} | ({"window_2k-1"} if K <= 32 else set()) | ({"unseeded"} if K > 2 else set())
        assert forms == want, (K, forms)
        if K > 2:
            assert {K - 1, K, K + 1} <= levels
        if 2 < K <= 32:
            assert {2 * K - 2, 2 * K - 1, 2 * K} <= levels


def test_the_guard_sees_a_dropped_and_an_added_size():
    sizes, sources = _header_sizes(), _sources()
    for f in PER_K_TESTS:
        cut = re.sub(r"(COMPILED_KS = \[.*?) 13,", r"\1", sources[f])
        assert cut != sources[f]
        bad = _untested(sizes, dict(sources, **{f: cut}))
        assert bad and all(b[0] == f and b[2] == [13] and b[3] == [] for b in bad) and len(bad) == len(PER_K_TESTS[f])
        # a test that leaves the shared list for a shorter literal one
        name = PER_K_TESTS[f][0]
        own = sources[f].replace('@pytest.mark.parametrize("K", COMPILED_KS)\ndef %s(' % name, '@pytest.mark.parametrize("K", [1, 16, 32])\ndef %s(' % name)
        assert own != sources[f] and [b[1] for b in _untested(sizes, dict(sources, **{f: own}))] == [name]
        # a per-K test that is gone
        gone = sources[f].replace("def %s(" % name, "def %s_off(" % name)
        assert [b[1] for b in _untested(sizes, dict(sources, **{f: gone}))] == [name]
    # a size compiled later: the header grows, the tests do not
    header = open(os.path.join(ROOT, "point-unet_amd", "csrc", "kdtree.h")).read()
    grown = header.replace("X(48) X(64)\n#endif", "X(48) X(64) X(96)\n#endif")
    assert grown != header and _header_sizes(grown) == sizes + [96]
    bad = _untested(_header_sizes(grown), sources)
    assert len(bad) == sum(len(v) for v in PER_K_TESTS.values()) and all(b[2] == [96] for b in bad)


def test_the_library_refuses_with_the_header_list(lib, dbg):
    """The refusals print the list they are compiled from: ps_debug_knn_host needs no device."""
    import numpy as np
    p = np.zeros((4, 3), np.float32)
    out = np.zeros((4, 17), np.int32)
    assert dbg.ps_debug_knn_host(p.ctypes.data, p.ctypes.data, 1, 4, 4, 17, out.ctypes.data) == 1
    msg = lib.ps_last_error().decode()
    assert [int(t) for t in msg.split("compiled sizes:")[1].rstrip(")").split()] == _header_sizes()
