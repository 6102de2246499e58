"""ctypes binding of tests/native/libupsample_reference.so — the CPU restatement of guided upsampling: the serial loop
over rt_amd/csrc/upsample_rules.hpp with the oracle's leaf functions, and rt_amd/csrc/upsample.cpp's checks and low-size rule.
TEST INFRASTRUCTURE.

Also here, shared by the CPU and the GPU tests: constructed guides (one constant hit surface, sky, random records)."""
from __future__ import annotations

import ctypes as C
import functools
import subprocess

import numpy as np

from rt_amd.capi import RtHipUpsampleParams
from tests.conftest import ROOT

LIBRARY = ROOT / "tests" / "native" / "libupsample_reference.so"
F32 = np.float32


@functools.lru_cache(maxsize=None)
def lib() -> C.CDLL:
    if not LIBRARY.exists():  # (`make` builds it with everything else; a tree that was never built gets it here)
        subprocess.run(["make", "-C", str(ROOT), str(LIBRARY.relative_to(ROOT))], check=True, capture_output=True)
    l = C.CDLL(str(LIBRARY))
    l.upsample_ref_default_params.restype = None
    l.upsample_ref_default_params.argtypes = [C.POINTER(RtHipUpsampleParams)]
    l.upsample_ref_check.restype = C.c_int
    l.upsample_ref_check.argtypes = [C.POINTER(RtHipUpsampleParams), C.c_char_p, C.c_size_t]
    l.upsample_ref_check_sizes.restype = C.c_int
    l.upsample_ref_check_sizes.argtypes = [C.c_uint32] * 4 + [C.c_char_p, C.c_size_t]
    l.upsample_ref_low_size.restype = C.c_int
    l.upsample_ref_low_size.argtypes = [C.c_uint32] * 3 + [C.POINTER(C.c_uint32)] * 2 + [C.c_char_p, C.c_size_t]
    l.upsample_ref_source_of.restype = None
    l.upsample_ref_source_of.argtypes = [C.c_uint32] * 3 + [C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_float)]
    l.upsample_ref_frame.restype = C.c_int
    l.upsample_ref_frame.argtypes = [C.c_uint32] * 4 + [C.c_void_p] * 3 + [C.POINTER(RtHipUpsampleParams), C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]
    return l


def params(**fields) -> RtHipUpsampleParams:
    """The defaults (default_upsample_params of rt_amd/csrc/upsample.cpp) with `fields` replaced."""
    p = RtHipUpsampleParams()
    lib().upsample_ref_default_params(C.byref(p))
    for name, value in fields.items():
        assert hasattr(p, name), name
        setattr(p, name, value)
    return p


def check(p: RtHipUpsampleParams):
    """check_upsample_params: (status, message)."""
    message = C.create_string_buffer(256)
    status = lib().upsample_ref_check(C.byref(p), message, len(message))
    return status, message.value.decode()


def check_sizes(W: int, H: int, w: int, h: int):
    message = C.create_string_buffer(256)
    status = lib().upsample_ref_check_sizes(W, H, w, h, message, len(message))
    return status, message.value.decode()


def low_size(W: int, H: int, factor: int):
    """upsample_low_size: (status, message, w, h)."""
    message = C.create_string_buffer(256)
    w, h = C.c_uint32(0), C.c_uint32(0)
    status = lib().upsample_ref_low_size(W, H, factor, C.byref(w), C.byref(h), message, len(message))
    return status, message.value.decode(), w.value, h.value


def source_of(x: int, W: int, w: int):
    """source_of: (first, b0, b1) with the weights as numpy float32."""
    first, b0, b1 = C.c_int32(0), C.c_float(0), C.c_float(0)
    lib().upsample_ref_source_of(x, W, w, C.byref(first), C.byref(b0), C.byref(b1))
    return first.value, F32(b0.value), F32(b1.value)


def frame(rgb_low: np.ndarray, guide_low: np.ndarray, guide_full: np.ndarray, p: RtHipUpsampleParams | None = None):
    """The whole reconstruction, serially: rgb_low float32[h, w, 3], guide_low float32[h, w, 8], guide_full float32[H, W, 8] ->
    (rgb float32[H, W, 3], rgba uint32[H, W], orphans)."""
    rgb_low = np.ascontiguousarray(rgb_low, dtype=F32)
    guide_low = np.ascontiguousarray(guide_low, dtype=F32)
    guide_full = np.ascontiguousarray(guide_full, dtype=F32)
    h, w = rgb_low.shape[:2]
    H, W = guide_full.shape[:2]
    assert rgb_low.shape == (h, w, 3) and guide_low.shape == (h, w, 8) and guide_full.shape == (H, W, 8)
    out = np.empty((H, W, 3), dtype=F32)
    rgba = np.empty((H, W), dtype=np.uint32)
    orphans = C.c_uint32(0)
    status = lib().upsample_ref_frame(W, H, w, h, rgb_low.ctypes.data, guide_low.ctypes.data, guide_full.ctypes.data, C.byref(p) if p is not None else None, out.ctypes.data, rgba.ctypes.data, C.byref(orphans))
    if status != 0:
        raise ValueError(f"upsample_ref_frame refused its arguments ({status})")
    return out, rgba, orphans.value


# ---- constructed guides ------------------------------------------------------------------------------------------------------------
def hit_guide(height: int, width: int, normal=(0.0, 0.0, 1.0), depth=2.0, albedo=(0.5, 0.5, 0.5), prim=1) -> np.ndarray:
    """One constant hit surface: every term of the weight but the bilinear one is exactly 1 between two such records."""
    g = np.zeros((height, width, 8), dtype=F32)
    g[..., 0:3] = normal
    g[..., 3] = depth
    g[..., 4:7] = albedo
    g[..., 7] = np.array([prim], dtype=np.uint32).view(F32)[0]
    return g


def sky_guide(height: int, width: int, colour=(0.5, 0.7, 1.0)) -> np.ndarray:
    g = np.zeros((height, width, 8), dtype=F32)
    g[..., 3] = -1.0
    g[..., 4:7] = colour
    return g


def random_guide(rng: np.random.Generator, height: int, width: int, sky_share=0.25) -> np.ndarray:
    """Random records: unit normals from a small set (so that neighbours often agree), depths in 1 .. 3, albedos from a small palette,
    a share of sky."""
    normals = np.array([[0, 0, 1], [0, 1, 0], [0.6, 0, 0.8], [0, 0.6, 0.8]], dtype=F32)
    palette = np.array([[0.5, 0.5, 0.5], [0.8, 0.3, 0.3], [0.52, 0.5, 0.48]], dtype=F32)
    g = np.zeros((height, width, 8), dtype=F32)
    g[..., 0:3] = normals[rng.integers(0, len(normals), size=(height, width))]
    g[..., 3] = rng.uniform(1.0, 3.0, size=(height, width)).astype(F32)
    g[..., 4:7] = palette[rng.integers(0, len(palette), size=(height, width))]
    ids = rng.integers(1, 6, size=(height, width)).astype(np.uint32)
    sky = rng.random((height, width)) < sky_share
    g[sky] = sky_guide(1, 1)[0, 0]
    ids[sky] = 0
    g[..., 7] = ids.view(F32)
    return g
