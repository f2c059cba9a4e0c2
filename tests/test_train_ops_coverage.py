"""Every op of the C surface is called by a GPU test.  The ps_op_* entries of include/pointseg_train_ops.h and include/pointseg.h are parsed
from the headers; each must be named in some tests/test_gpu_*.py -- the training ops directly (tests/test_gpu_train_ops.py holds the ones
the whole-step tests only reach from inside the trainer).  Five inference ops are reached through a package wrapper instead: WRAPPED names
the wrapper and the GPU test that calls it, and both links are checked in the sources."""
import ast
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# op -> (package file, wrapper function, name the test calls it by, GPU test file, test function)
WRAPPED = {
    "ps_op_att_pool": ("RandLANet.py", "att_pooling", "att_pooling", "test_gpu_grid_ops.py", "test_op_by_op_surface_vs_oracle"),
    "ps_op_half_to_float": ("RandLANet.py", "inference", "inference", "test_gpu_network.py", "test_half_precision_feature_input"),
    "ps_op_nearest_interpolation": ("RandLANet.py", "nearest_interpolation", "nearest_interpolation", "test_gpu_grid_ops.py",
                                    "test_op_by_op_surface_vs_oracle"),
    "ps_op_probs_to_volume": ("postprocess.py", "point2prod", "point2prod", "test_gpu_grid_ops.py",
                              "test_point_to_volume_scatter_matches_the_reference_loop"),
    "ps_op_relative_pos_encoding": ("RandLANet.py", "relative_pos_encoding", "relative_pos_encoding", "test_gpu_grid_ops.py",
                                    "test_op_by_op_surface_vs_oracle"),
}
# the training ops no test called before tests/test_gpu_train_ops.py
TRAIN_OPS_ADDED = ["ps_op_adam", "ps_op_dropout", "ps_op_mul", "ps_op_axpy", "ps_op_add_lrelu_bwd", "ps_op_bn_train_sums", "ps_op_bn_train_apply",
                   "ps_op_bn_train_apply_ex", "ps_op_bn_train_bwd_sums", "ps_op_bn_train_bwd_sums_ex", "ps_op_bn_train_bwd_apply",
                   "ps_op_bn_train_bwd_apply_ex", "ps_op_bn_train_fwd_mov", "ps_op_conv_bn_train_bwd_sums", "ps_op_conv_bn_train_bwd_apply",
                   "ps_op_conv_bn_train_supported"]


def _declared(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    return re.findall(r"^(?:int|int64_t)\s+(ps_op_\w+)\s*\(", src, re.M)


def _gpu_test_sources():
    return {os.path.basename(f): open(f).read() for f in sorted(glob.glob(os.path.join(ROOT, "tests", "test_gpu_*.py")))}


def _missing(ops, sources):
    return [op for op in ops if op not in WRAPPED and not any(re.search(r"\b%s\b" % op, s) for s in sources.values())]


def _function(src, name):
    """Source of the function (or method) `name` in module source `src`, or None."""
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, ast.FunctionDef) and node.name == name:
            return ast.get_source_segment(src, node)
    return None


def test_the_headers_parse():
    train, infer = _declared("pointseg_train_ops.h"), _declared("pointseg.h")
    assert len(train) == len(set(train)) >= 60 and len(infer) == len(set(infer)) >= 8
    assert set(TRAIN_OPS_ADDED) <= set(train) and set(WRAPPED) <= set(infer)


def test_every_training_op_is_called_by_a_gpu_test():
    missing = _missing(_declared("pointseg_train_ops.h"), _gpu_test_sources())
    assert not missing, "ops of include/pointseg_train_ops.h that no tests/test_gpu_*.py calls: %s" % missing


def test_every_inference_op_is_called_by_a_gpu_test_or_through_its_wrapper():
    missing = _missing(_declared("pointseg.h"), _gpu_test_sources())
    assert not missing, "ops of include/pointseg.h that no tests/test_gpu_*.py calls (add a test, or a WRAPPED entry): %s" % missing


def test_each_wrapper_calls_its_op_and_its_gpu_test_calls_the_wrapper():
    sources = _gpu_test_sources()
    for op, (module, wrapper, called_as, test_file, test_name) in WRAPPED.items():
        body = _function(open(os.path.join(ROOT, "point-unet_amd", module)).read(), wrapper)
        assert body is not None, (op, module, wrapper)
        assert re.search(r"\b%s\(" % op, body), "%s.%s does not call %s" % (module, wrapper, op)
        test = _function(sources[test_file], test_name)
        assert test is not None, (op, test_file, test_name)
        assert re.search(r"\b%s\(" % called_as, test), "%s::%s does not call %s" % (test_file, test_name, called_as)
        assert "pytest.mark.gpu" in sources[test_file]


def test_the_guard_sees_a_removed_op():
    """Taking any one of the ops tests/test_gpu_train_ops.py added out of the GPU tests fails the guard above (the other ops stay found)."""
    sources = _gpu_test_sources()
    train = _declared("pointseg_train_ops.h")
    assert _missing(train, sources) == []
    for op in TRAIN_OPS_ADDED:
        cut = {name: re.sub(r"\b%s\b" % op, "ps_op_removed", s) for name, s in sources.items()}
        assert _missing(train, cut) == [op], op
