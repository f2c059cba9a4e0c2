"""Every experiment knob of struct ps::Tuning (csrc/common.h) picks between shipped kernels, and the default library never changes one
(test_host_logic.py::test_the_default_library_never_reads_the_environment).  So the non-default branches only run where a test sets the
knob on its own context through the test door ps_debug_set_tuning (tests/tuning.py).  These CPU tests keep that door and the GPU tests
of tests/test_gpu_tuning_paths.py in step with the struct: a knob added later without a test fails here."""
import ast
import os
import re

import tuning

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOT_A_PATH = {"wgrad_debug"}  # (prints shapes, computes nothing)


def _struct():
    """[(field, default value)] of struct Tuning, in order."""
    src = open(os.path.join(ROOT, "point-unet_amd", "csrc", "common.h")).read()
    body = re.search(r"struct Tuning \{(.*?)\n\};", src, re.S).group(1)
    out = []
    for line in body.splitlines():
        code = line.split("//")[0].strip()
        if not code:
            continue
        m = re.match(r"(?:bool|int|int64_t|double)\s+(.*);$", code)
        assert m, "unparsed line of struct Tuning: %r" % line
        for decl in m.group(1).split(","):
            name, value = (t.strip() for t in decl.split("="))
            out.append((name, float(eval(value.replace("true", "1").replace("false", "0"), {"__builtins__": {}}))))
    return out


def _struct_fields():
    return [n for n, _ in _struct()]


def _constant(node):
    """The value of a constant expression (numbers, unary minus, arithmetic, shifts), or None when it is not one (a loop variable)."""
    if not all(isinstance(n, (ast.Expression, ast.Constant, ast.UnaryOp, ast.BinOp, ast.operator, ast.unaryop)) for n in ast.walk(ast.Expression(node))):
        return None
    return float(eval(compile(ast.Expression(node), "<knob>", "eval"), {"__builtins__": {}}))


def _knobs_set(sources):
    """Knobs a test source really sets to a non-default value: keywords of tuned_context(...), entries of knob dicts (the parametrize
    lists that feed tuned_context(**knobs)) and set_tuning(ctx, "name", value) calls.  A value that is an expression of loop variables
    counts; a constant counts only when it differs from the shipped default.  Not counted: reading a knob (knobs.get, get_tuning) and the
    values test_the_door_refuses_values_the_kernels_are_not_compiled_for hands to the door to be refused."""
    defaults = dict(_struct())
    found = set()

    def real(name, value):
        if name in defaults:
            v = _constant(value)
            if v is None or v != defaults[name]:
                found.add(name)

    def visit(node):
        if isinstance(node, ast.FunctionDef) and node.name.startswith("test_the_door_refuses"):
            return
        if isinstance(node, ast.Call):
            fn = node.func.id if isinstance(node.func, ast.Name) else getattr(node.func, "attr", "")
            if fn == "tuned_context":
                for kw in node.keywords:
                    if kw.arg:
                        real(kw.arg, kw.value)
            elif fn == "set_tuning" and len(node.args) >= 3 and isinstance(node.args[1], ast.Constant):
                real(node.args[1].value, node.args[2])
        elif isinstance(node, ast.Dict):
            for k, v in zip(node.keys, node.values):
                if isinstance(k, ast.Constant) and isinstance(k.value, str):
                    real(k.value, v)
        for child in ast.iter_child_nodes(node):
            visit(child)

    for src in sources:
        visit(ast.parse(src))
    return found


def _test_sources():
    return [open(os.path.join(ROOT, "tests", f)).read() for f in ("test_gpu_tuning_paths.py", "syncbn_worker.py")]


def test_the_struct_parses():
    names = _struct_fields()
    assert len(names) == len(set(names)) >= 20
    assert {"inv_tile", "gemm32b_rw", "gemm32b_cw", "train_merge_syncbn", "wgrad_debug"} <= set(names)


def test_the_tuning_door_knows_every_field(dbg):
    assert tuning.fields() == _struct_fields()


def test_the_tuning_door_refuses_without_a_context(dbg, lib):
    import ctypes
    assert tuning.dbg().ps_debug_set_tuning(None, b"inv_tile", 6144.0) != 0 and b"NULL" in lib.ps_last_error()
    assert tuning.dbg().ps_debug_gemm32_plan(None, 0, 32, 64, 64, (ctypes.c_int * 4)()) != 0
    assert tuning.dbg().ps_debug_tuning_fields(ctypes.create_string_buffer(8), 8) != 0


def test_every_knob_is_set_by_a_gpu_test():
    """tests/test_gpu_tuning_paths.py (and tests/syncbn_worker.py, for train_merge_syncbn) set every knob to a value other than the
    shipped one -- see _knobs_set for what counts as setting."""
    missing = [n for n in _struct_fields() if n not in NOT_A_PATH and n not in _knobs_set(_test_sources())]
    assert not missing, "knobs of struct Tuning that no GPU test sets: %s" % missing


def test_the_coverage_guard_sees_a_removed_setting():
    """The guard above fails when a setting goes: without the two att64_occ entries of the pooling test's parametrize list, or with the
    worker's train_merge_syncbn = 0 turned into the default 1.  Refused values, read-backs and resets to the default do not count."""
    gpu, worker = _test_sources()
    assert "att64_occ" in _knobs_set([gpu])
    cut = re.sub(r"\(\"\w+\", \{\"att64_occ\": \d\}\),?", "", gpu)
    assert cut != gpu and "att64_occ" not in _knobs_set([cut, worker])
    assert "train_merge_syncbn" in _knobs_set([worker])
    flipped = worker.replace('"train_merge_syncbn", 0)', '"train_merge_syncbn", 1)')
    assert flipped != worker and "train_merge_syncbn" not in _knobs_set([gpu, flipped])
    decoys = """
def test_the_door_refuses_values_the_kernels_are_not_compiled_for():
    for name, bad in [("att64_occ", 3), ("convbn_max_c", 4097), ("bn_slice", 0.5)]:
        set_tuning(ctx, name, bad)
def other(knobs, ctx):
    if knobs.get("inv_bucket", 1) and get_tuning(ctx, "wgrad_wgs") == 512:
        set_tuning(ctx, "train_merge_syncbn", 1)
    with tuned_context(inv_tile=4096, bn_slice=False) as c:
        pass
"""
    assert _knobs_set([decoys]) == set()
