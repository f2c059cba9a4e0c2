"""Test-side bindings of the experiment-knob doors of the TEST-ONLY library libpointseg_debug.so (csrc/debug_hooks.h): ps_debug_set_tuning /
ps_debug_get_tuning / ps_debug_tuning_fields (the fields of struct ps::Tuning, csrc/common.h, by C++ name) and ps_debug_gemm32_plan (the launch
gemm32() / gemm32b() make).  tuned_context() gives a FRESH runtime.Context with the knobs set, so the session's default context -- which
every other test shares -- never holds anything but the shipped values."""
import contextlib
import ctypes
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_h = None


def dbg():
    global _h
    if _h is None:
        from point_unet_amd import _lib
        _lib.lib()  # the product library first: the debug library links against it
        h = ctypes.CDLL(os.path.join(ROOT, "point-unet_amd", "libpointseg_debug.so"))
        c_vp, c_int = ctypes.c_void_p, ctypes.c_int
        for name, args in {
            "ps_debug_set_tuning": [c_vp, ctypes.c_char_p, ctypes.c_double],
            "ps_debug_get_tuning": [c_vp, ctypes.c_char_p, ctypes.POINTER(ctypes.c_double)],
            "ps_debug_tuning_fields": [ctypes.c_char_p, c_int],
            "ps_debug_gemm32_plan": [c_vp, c_int, ctypes.c_int64, c_int, c_int, ctypes.POINTER(c_int)],
        }.items():
            fn = getattr(h, name)
            fn.restype = c_int
            fn.argtypes = args
        _h = h
    return _h


def _check(rc):
    from point_unet_amd import _lib
    _lib.check(rc)


def fields():
    """Every knob name the doors know, in struct order."""
    buf = ctypes.create_string_buffer(4096)
    _check(dbg().ps_debug_tuning_fields(buf, len(buf)))
    return buf.value.decode().split()


def set_tuning(ctx, name, value):
    _check(dbg().ps_debug_set_tuning(ctx.handle, name.encode(), float(value)))


def get_tuning(ctx, name):
    v = ctypes.c_double()
    _check(dbg().ps_debug_get_tuning(ctx.handle, name.encode(), ctypes.byref(v)))
    return v.value


def gemm32_plan(ctx, split_bf16, R, cin, cout):
    """(rw, cw, sk, pd) of the launch ps_debug_gemm32 makes on `ctx` for R x cin x cout."""
    out = (ctypes.c_int * 4)()
    _check(dbg().ps_debug_gemm32_plan(ctx.handle, int(split_bf16), int(R), int(cin), int(cout), out))
    return tuple(out)


@contextlib.contextmanager
def tuned_context(**knobs):
    """A fresh runtime.Context on torch's current device and stream with `knobs` set (and read back); closed on exit.  The trainer reads
    its train_* knobs when it is created: create it inside the block."""
    import torch
    from point_unet_amd import runtime
    ctx = runtime.Context(torch.cuda.current_device())
    try:
        ctx.use_torch_stream()
        for name, value in knobs.items():
            set_tuning(ctx, name, value)
            assert get_tuning(ctx, name) == float(value), name
        yield ctx
    finally:
        torch.cuda.synchronize()
        ctx.close()
