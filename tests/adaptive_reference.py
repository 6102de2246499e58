"""ctypes binding of tests/native/libadaptive_reference.so — the CPU restatement of adaptive sampling's update step:
the serial loop over rt_amd/csrc/adaptive_rules.hpp, every pixel finished with the oracle's pack, and rt_amd/csrc/adaptive.cpp's
defaults and parameter check.  TEST INFRASTRUCTURE, shared by the CPU and the GPU tests."""
from __future__ import annotations

import ctypes as C
import functools
import subprocess

import numpy as np

from rt_amd.capi import RtHipAdaptiveParams
from tests.conftest import ROOT

LIBRARY = ROOT / "tests" / "native" / "libadaptive_reference.so"
F32 = np.float32
STOPPED = np.uint32(0x80000000)
COUNT = np.uint32(0x7FFFFFFF)


@functools.lru_cache(maxsize=None)
def lib() -> C.CDLL:
    if not LIBRARY.exists():  # (`make` builds it with everything else; a tree that was never built gets it here)
        subprocess.run(["make", "-C", str(ROOT), str(LIBRARY.relative_to(ROOT))], check=True, capture_output=True)
    l = C.CDLL(str(LIBRARY))
    l.adaptive_ref_default_params.restype = None
    l.adaptive_ref_default_params.argtypes = [C.POINTER(RtHipAdaptiveParams)]
    l.adaptive_ref_pass_size.restype = C.c_uint64
    l.adaptive_ref_pass_size.argtypes = [C.c_uint32]
    l.adaptive_ref_check.restype = C.c_int
    l.adaptive_ref_check.argtypes = [C.POINTER(RtHipAdaptiveParams), C.c_uint64, C.c_char_p, C.c_size_t]
    l.adaptive_ref_step.restype = C.c_int
    l.adaptive_ref_step.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(RtHipAdaptiveParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]
    return l


def params(**fields) -> RtHipAdaptiveParams:
    """The defaults (default_adaptive_params of rt_amd/csrc/adaptive.cpp) with `fields` replaced."""
    p = RtHipAdaptiveParams()
    lib().adaptive_ref_default_params(C.byref(p))
    for name, value in fields.items():
        assert hasattr(p, name), name
        setattr(p, name, value)
    return p


def pass_size(pass_samples: int) -> int:
    return int(lib().adaptive_ref_pass_size(pass_samples))


def check(p: RtHipAdaptiveParams, size: int = 16):
    """check_adaptive_params against a pass size: (status, message)."""
    message = C.create_string_buffer(256)
    status = lib().adaptive_ref_check(C.byref(p), size, message, len(message))
    return status, message.value.decode()


def step(accum, pass_sum, moments, state, pass_samples: int, first_pass: bool, whole_pass: bool = True, p: RtHipAdaptiveParams | None = None):
    """One whole update step, serially — rt_hip_adaptive_update_device's arguments on host arrays of a height x width frame.  Returns
    (moments float32[H, W, 2], state uint32[H, W], rgba uint32[H, W], rgb float32[H, W, 3], active pixels); the inputs are left alone."""
    accum = np.ascontiguousarray(accum, dtype=F32)
    pass_sum = np.ascontiguousarray(pass_sum, dtype=F32)
    height, width = accum.shape[:2]
    assert accum.shape == (height, width, 3) and pass_sum.shape == accum.shape
    moments = np.array(moments, dtype=F32, copy=True, order="C")
    state = np.array(state, dtype=np.uint32, copy=True, order="C")
    assert moments.shape == (height, width, 2) and state.shape == (height, width)
    rgba = np.empty((height, width), dtype=np.uint32)
    rgb = np.empty((height, width, 3), dtype=F32)
    active = C.c_uint32()
    with np.errstate(all="ignore"):
        status = lib().adaptive_ref_step(width, height, pass_samples, int(bool(first_pass)), int(bool(whole_pass)), C.byref(p) if p is not None else None, accum.ctypes.data, pass_sum.ctypes.data, moments.ctypes.data, state.ctypes.data,
                                         rgba.ctypes.data, rgb.ctypes.data, C.byref(active))
    if status != 0:
        raise ValueError(f"adaptive_ref_step refused its arguments ({status})")
    return moments, state, rgba, rgb, active.value
