"""ctypes binding of tests/native/libbloom_reference.so — the CPU restatement of bloom: the serial loops over
rt_amd/csrc/bloom_rules.hpp, and rt_amd/csrc/bloom.cpp's check, level plan and parser.  TEST INFRASTRUCTURE.

Also here, shared by the CPU and the GPU tests: the noise frames and the constructed frames (flat colours, impulses in the corners and
the middle, hostile pixels among bright ones, denormals)."""
from __future__ import annotations

import ctypes as C
import functools
import subprocess

import numpy as np

from rt_amd.capi import RtHipBloomParams
from tests.conftest import ROOT

LIBRARY = ROOT / "tests" / "native" / "libbloom_reference.so"
F32 = np.float32
MAX_LEVELS = 8
CAP = 2.0 ** 20


@functools.lru_cache(maxsize=None)
def lib() -> C.CDLL:
    if not LIBRARY.exists():  # (`make` builds it with everything else; a tree that was never built gets it here)
        subprocess.run(["make", "-C", str(ROOT), str(LIBRARY.relative_to(ROOT))], check=True, capture_output=True)
    l = C.CDLL(str(LIBRARY))
    l.bloom_ref_default_params.restype = None
    l.bloom_ref_default_params.argtypes = [C.POINTER(RtHipBloomParams)]
    l.bloom_ref_check.restype = C.c_int
    l.bloom_ref_check.argtypes = [C.POINTER(RtHipBloomParams), C.c_char_p, C.c_size_t]
    l.bloom_ref_from_spec.restype = C.c_int
    l.bloom_ref_from_spec.argtypes = [C.c_char_p, C.POINTER(RtHipBloomParams), C.c_char_p, C.c_size_t]
    l.bloom_ref_plan.restype = C.c_int
    l.bloom_ref_plan.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(RtHipBloomParams), C.POINTER(C.c_uint32), C.c_void_p, C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_uint64)]
    l.bloom_ref_frame.restype = C.c_int
    l.bloom_ref_frame.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(RtHipBloomParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return l


def params(**fields) -> RtHipBloomParams:
    """The defaults (default_bloom_params of rt_amd/csrc/bloom.cpp) with `fields` replaced."""
    p = RtHipBloomParams()
    lib().bloom_ref_default_params(C.byref(p))
    for name, value in fields.items():
        assert hasattr(p, name), name
        setattr(p, name, value)
    return p


def check(p: RtHipBloomParams):
    """check_bloom_params: (status, message)."""
    message = C.create_string_buffer(256)
    status = lib().bloom_ref_check(C.byref(p), message, len(message))
    return status, message.value.decode()


def from_spec(spec: bytes):
    """bloom_from_spec: (status, message, params)."""
    message = C.create_string_buffer(256)
    p = RtHipBloomParams()
    status = lib().bloom_ref_from_spec(spec, C.byref(p), message, len(message))
    return status, message.value.decode(), p


def plan(width: int, height: int, p: RtHipBloomParams | None = None) -> dict:
    """plan_bloom: sizes [(w, h)] per level, offsets in floats, norm and gain as float32, scratch_bytes."""
    levels, norm, gain, scratch = C.c_uint32(), C.c_float(), C.c_float(), C.c_uint64()
    sizes, offsets = np.zeros(2 * MAX_LEVELS, dtype=np.uint32), np.zeros(MAX_LEVELS, dtype=np.uint64)
    status = lib().bloom_ref_plan(width, height, C.byref(p) if p is not None else None, C.byref(levels), sizes.ctypes.data, offsets.ctypes.data, C.byref(norm), C.byref(gain), C.byref(scratch))
    if status != 0:
        raise ValueError(f"bloom_ref_plan refused its arguments ({status})")
    n = levels.value
    return {"levels": n, "sizes": [(int(sizes[2 * i]), int(sizes[2 * i + 1])) for i in range(n)], "offsets": [int(o) for o in offsets[:n]], "norm": F32(norm.value), "gain": F32(gain.value), "scratch_bytes": int(scratch.value)}


def frame(rgb: np.ndarray, p: RtHipBloomParams | None = None, want_levels: bool = False):
    """The whole operation, serially: rgb float32[H, W, 3] -> (out float32[H, W, 3], layer float32[H, W, 3]) and, with want_levels,
    two lists of float32[h, w, 3]: every level as the way down left it and as the way up left it.  `rgb` is not modified."""
    rgb = np.ascontiguousarray(rgb, dtype=F32)
    H, W = rgb.shape[:2]
    assert rgb.shape == (H, W, 3)
    out, layer = np.empty((H, W, 3), dtype=F32), np.empty((H, W, 3), dtype=F32)
    pl = plan(W, H, p)
    down = np.empty(pl["scratch_bytes"] // 4, dtype=F32) if want_levels else None
    up = np.empty(pl["scratch_bytes"] // 4, dtype=F32) if want_levels else None
    status = lib().bloom_ref_frame(W, H, rgb.ctypes.data, C.byref(p) if p is not None else None, down.ctypes.data if want_levels else None, up.ctypes.data if want_levels else None, layer.ctypes.data, out.ctypes.data)
    if status != 0:
        raise ValueError(f"bloom_ref_frame refused its arguments ({status})")
    if not want_levels:
        return out, layer
    cut = lambda block: [block[o:o + 3 * w * h].reshape(h, w, 3) for (w, h), o in zip(pl["sizes"], pl["offsets"])]
    return out, layer, cut(down), cut(up)


# ---- frames -------------------------------------------------------------------------------------------------------------------------
def noise(height: int, width: int, seed: int = 7) -> np.ndarray:
    """Positive noise: channels uniform in [0.01, 0.9), and a tenth of the pixels lifted above the default threshold, by 2 .. 64."""
    rng = np.random.default_rng(seed)
    rgb = rng.uniform(0.01, 0.9, size=(height, width, 3))
    bright = rng.random((height, width)) < 0.1
    rgb[bright] *= np.exp2(rng.uniform(1.0, 6.0, size=(int(bright.sum()), 1))) / 0.45
    return rgb.astype(F32)


def flat(height: int, width: int, colour=(2.0, 3.0, 4.0)) -> np.ndarray:
    return np.broadcast_to(np.array(colour, dtype=F32), (height, width, 3)).copy()


FLAT_PARAMS = dict(threshold=1.0, knee=0.0, scatter=0.5)  # every tap sum of a flat (2, 3, 4) frame is exact under these


def impulse(height: int, width: int, y: int, x: int, value: float = 8.0) -> np.ndarray:
    rgb = np.zeros((height, width, 3), dtype=F32)
    rgb[y, x] = [value, value / 2, value / 4]
    return rgb


def hostile(height: int = 21, width: int = 37):
    """(the frame with a NaN, a +inf and a negative pixel among bright ones; the same frame with those channels as the bright pass
    takes them: 0, 2^20, 0; the NaN pixel's (y, x))."""
    rgb = noise(height, width, seed=5)
    rgb[3:9, 4:12] *= 8  # bright ones around them
    clean = rgb.copy()
    rgb[5, 6] = [np.nan, 3.0, 5.0]
    clean[5, 6] = [0.0, 3.0, 5.0]
    rgb[6, 9] = [np.inf, 2.0, 1.0]
    clean[6, 9] = [CAP, 2.0, 1.0]
    rgb[4, 5] = [-7.0, 6.0, -0.0]
    clean[4, 5] = [0.0, 6.0, 0.0]
    return rgb, clean, (5, 6)


def constructed_cases() -> dict:
    """name -> (rgb float32[H, W, 3], RtHipBloomParams): small ragged frames, shared by the CPU and the GPU tests."""
    cases = {}
    for height, width in ((1, 1), (3, 5), (21, 37)):
        cases[f"flat {width}x{height}"] = (flat(height, width), params(**FLAT_PARAMS))
    H, W = 21, 37
    for name, (y, x) in {"top left": (0, 0), "top right": (0, W - 1), "bottom left": (H - 1, 0), "bottom right": (H - 1, W - 1), "middle": (H // 2, W // 2)}.items():
        cases[f"impulse {name}"] = (impulse(H, W, y, x), params(threshold=1.0, knee=0.5, scatter=1.0, levels=8))
    bad, clean, _ = hostile()
    cases["hostile pixels"] = (bad, params())
    cases["hostile pixels, as the bright pass takes them"] = (clean, params())
    rng = np.random.default_rng(3)
    cases["denormals"] = ((rng.uniform(0.5, 9.0, size=(9, 13, 3)) * 1e-39).astype(F32), params(threshold=0.0, knee=0.0, intensity=1.0))
    return cases
