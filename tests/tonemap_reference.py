"""ctypes binding of tests/native/libtonemap_reference.so — the CPU restatement of tone mapping: the serial loops over
rt_amd/csrc/tonemap_rules.hpp with the oracle's square root and pack, and rt_amd/csrc/tonemap.cpp's check and parser.
TEST INFRASTRUCTURE.

Also here, shared by the CPU and the GPU tests: the fixtures' float frames and the constructed frames (every pixel in one bin, every
pixel skipped, the end bins, rank cuts inside a bin and on a bin's edge, a single metered pixel, hostile channels)."""
from __future__ import annotations

import ctypes as C
import functools
import subprocess

import numpy as np

from rt_amd.capi import RtHipTonemapParams
from tests.conftest import ROOT

LIBRARY = ROOT / "tests" / "native" / "libtonemap_reference.so"
F32 = np.float32
STATE_WORDS = 8
NONE, REINHARD, ACES = 0, 1, 2
CURVES = (NONE, REINHARD, ACES)


@functools.lru_cache(maxsize=None)
def lib() -> C.CDLL:
    if not LIBRARY.exists():  # (`make` builds it with everything else; a tree that was never built gets it here)
        subprocess.run(["make", "-C", str(ROOT), str(LIBRARY.relative_to(ROOT))], check=True, capture_output=True)
    l = C.CDLL(str(LIBRARY))
    l.tonemap_ref_default_params.restype = None
    l.tonemap_ref_default_params.argtypes = [C.POINTER(RtHipTonemapParams)]
    l.tonemap_ref_check.restype = C.c_int
    l.tonemap_ref_check.argtypes = [C.POINTER(RtHipTonemapParams), C.c_char_p, C.c_size_t]
    l.tonemap_ref_from_spec.restype = C.c_int
    l.tonemap_ref_from_spec.argtypes = [C.c_char_p, C.POINTER(RtHipTonemapParams), C.c_char_p, C.c_size_t]
    l.tonemap_ref_histogram.restype = None
    l.tonemap_ref_histogram.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p]
    l.tonemap_ref_frame.restype = C.c_int
    l.tonemap_ref_frame.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(RtHipTonemapParams), C.c_void_p, C.c_void_p, C.c_void_p]
    return l


def params(**fields) -> RtHipTonemapParams:
    """The defaults (default_tonemap_params of rt_amd/csrc/tonemap.cpp) with `fields` replaced."""
    p = RtHipTonemapParams()
    lib().tonemap_ref_default_params(C.byref(p))
    for name, value in fields.items():
        assert hasattr(p, name), name
        setattr(p, name, value)
    return p


def check(p: RtHipTonemapParams):
    """check_tonemap_params: (status, message)."""
    message = C.create_string_buffer(256)
    status = lib().tonemap_ref_check(C.byref(p), message, len(message))
    return status, message.value.decode()


def from_spec(spec: bytes):
    """tonemap_from_spec: (status, message, params)."""
    message = C.create_string_buffer(256)
    p = RtHipTonemapParams()
    status = lib().tonemap_ref_from_spec(spec, C.byref(p), message, len(message))
    return status, message.value.decode(), p


def histogram(rgb: np.ndarray) -> np.ndarray:
    """The meter's 257 words for a float frame: 256 bins, then the skipped pixels."""
    rgb = np.ascontiguousarray(rgb, dtype=F32).reshape(-1, 3)
    out = np.zeros(257, dtype=np.uint32)
    lib().tonemap_ref_histogram(len(rgb), rgb.ctypes.data, out.ctypes.data)
    return out


def frame(rgb: np.ndarray, p: RtHipTonemapParams | None = None, state: np.ndarray | None = None):
    """The whole operation, serially: rgb float32[H, W, 3] -> (mapped float32[H, W, 3], rgba uint32[H, W], state uint32[8]).
    `state`: the record of the call before (None: zeroed); it is not modified."""
    rgb = np.ascontiguousarray(rgb, dtype=F32)
    H, W = rgb.shape[:2]
    assert rgb.shape == (H, W, 3)
    record = np.zeros(STATE_WORDS, dtype=np.uint32) if state is None else np.array(state, dtype=np.uint32)
    out = np.empty((H, W, 3), dtype=F32)
    rgba = np.empty((H, W), dtype=np.uint32)
    status = lib().tonemap_ref_frame(W, H, rgb.ctypes.data, C.byref(p) if p is not None else None, record.ctypes.data, out.ctypes.data, rgba.ctypes.data)
    if status != 0:
        raise ValueError(f"tonemap_ref_frame refused its arguments ({status})")
    return out, rgba, record


def info_of(state: np.ndarray) -> dict:
    """The state record as rt_hip_tonemap_info reports it."""
    words = np.asarray(state, dtype=np.uint32)
    return {"exposure": float(words[:1].view(F32)[0]), "target": float(words[1:2].view(F32)[0]), "counted": int(words[2]), "skipped": int(words[3]), "kept": int(words[4]), "mean_q8": int(words[5])}


# ---- frames -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fixture_frames() -> dict:
    """The float means of the committed fixtures: the lights scene (mean far above 1) under both scatter tables, and the basic scene."""
    golden = ROOT / "tests" / "golden"
    lights, basic = np.load(golden / "lights_64x36_spp20.npz"), np.load(golden / "basic_64x36_spp4.npz")
    return {"lights": lights["rgb"].astype(F32), "lights_sm": lights["rgb_sm"].astype(F32), "basic": basic["rgb"].astype(F32)}


def noise(height: int, width: int, seed: int = 7, low: float = -20.0, high: float = 20.0) -> np.ndarray:
    """Channels 2^u, u uniform in [low, high): every bin and both end bins are met."""
    rng = np.random.default_rng(seed)
    return np.exp2(rng.uniform(low, high, size=(height, width, 3))).astype(F32)


def grey(height: int, width: int, values) -> np.ndarray:
    """A grey frame whose pixels (row-major) cycle through `values`: the luminance of grey v is within an ulp or two of v."""
    values = np.asarray(values, dtype=F32)
    flat = values[np.arange(height * width) % len(values)]
    return np.repeat(flat.reshape(height, width, 1), 3, axis=2).copy()


def bin_centre(b: int) -> float:
    """A luminance in the middle of bin b (far from its edges, so that a grey pixel of that value lands in b whatever the last bits)."""
    return float(np.array([((888 + b) << 20) + (1 << 19)], dtype=np.uint32).view(F32)[0])


def constructed_cases() -> dict:
    """name -> (rgb float32[H, W, 3], RtHipTonemapParams).  Small ragged frames (35 pixels: no multiple of 4)."""
    nan, inf = float("nan"), float("inf")
    H, W = 5, 7
    cases = {}
    cases["one bin"] = (grey(H, W, [bin_centre(100)]), params())
    skipped = grey(H, W, [nan, 0.0, -1.0, inf])
    cases["all skipped"] = (skipped, params())
    cases["end bins"] = (grey(H, W, [1e-30, 2.0 ** -17, 2.0 ** 17, 3e38]), params(low_permille=0, high_permille=0))
    # 35 pixels, 20 in bin 60 and 15 in bin 200 (cycling 7 values: 4 + 3): low = 100 permille drops floor(3.5) = 3 inside bin 60
    two = grey(H, W, [bin_centre(60)] * 4 + [bin_centre(200)] * 3)
    cases["cut inside a bin"] = (two, params(low_permille=100, high_permille=100))
    # 40 pixels, 10 in each of four bins: 250 permille drops exactly the first bin, 250 exactly the last
    four = grey(5, 8, [bin_centre(40), bin_centre(80), bin_centre(120), bin_centre(160)])
    cases["cut on a bin edge"] = (four, params(low_permille=250, high_permille=250))
    cases["no trim"] = (two, params(low_permille=0, high_permille=0))
    one = grey(H, W, [nan])
    one[2, 3] = bin_centre(77)
    cases["one metered pixel, 999 permille"] = (one, params(low_permille=500, high_permille=499))
    cases["min clamp"] = (grey(H, W, [1000.0]), params(min_exposure=0.5, max_exposure=2.0))
    cases["max clamp"] = (grey(H, W, [0.001]), params(min_exposure=0.5, max_exposure=2.0))
    cases["manual exposure"] = (noise(H, W, seed=3), params(exposure=0.37))
    hostile = noise(H, W, seed=5, low=-4.0, high=4.0)
    hostile[0, 0] = [nan, 1.0, 2.0]
    hostile[0, 1] = [inf, 0.5, 0.25]
    hostile[0, 2] = [-3.0, 4.0, -0.0]
    hostile[0, 3] = [2.0 ** 21, 2.0 ** 20, 3e38]
    hostile[0, 4] = [-inf, nan, inf]
    hostile[0, 5] = [0.0, 0.0, 0.0]
    for curve, name in zip(CURVES, ("none", "reinhard", "aces")):
        cases[f"hostile channels, {name}"] = (hostile, params(curve=curve, exposure=1.0))
        cases[f"hostile channels metered, {name}"] = (hostile, params(curve=curve))
    return cases
