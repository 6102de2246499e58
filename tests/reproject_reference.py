"""ctypes binding of tests/native/libreproject_reference.so — the CPU restatement of temporal accumulation: the serial
loop over rt_amd/csrc/reproject_rules.hpp with the oracle's leaf functions and oracle_primary_ray, and rt_amd/csrc/temporal.cpp's
parameter check, forward_view_projection and same_history.  TEST INFRASTRUCTURE.

Also here, shared by the CPU and the GPU tests and by tools/temporal_tune.py: `sequence`, which blends a list of frames the way
rt_hip_render_temporal does (guide, reprojection, ping-pong), composed from the oracle and the two restatements."""
from __future__ import annotations

import ctypes as C
import functools
import subprocess

import numpy as np

from rt_amd.capi import RtHipScene, RtHipTemporalParams
from tests.conftest import ROOT

LIBRARY = ROOT / "tests" / "native" / "libreproject_reference.so"
F32 = np.float32


@functools.lru_cache(maxsize=None)
def lib() -> C.CDLL:
    if not LIBRARY.exists():  # (`make` builds it with everything else; a tree that was never built gets it here)
        subprocess.run(["make", "-C", str(ROOT), str(LIBRARY.relative_to(ROOT))], check=True, capture_output=True)
    l = C.CDLL(str(LIBRARY))
    l.reproject_ref_default_params.restype = None
    l.reproject_ref_default_params.argtypes = [C.POINTER(RtHipTemporalParams)]
    l.reproject_ref_check.restype = C.c_int
    l.reproject_ref_check.argtypes = [C.POINTER(RtHipTemporalParams), C.c_char_p, C.c_size_t]
    l.reproject_ref_forward.restype = C.c_int
    l.reproject_ref_forward.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
    key = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32]
    l.reproject_ref_same_history.restype = C.c_int
    l.reproject_ref_same_history.argtypes = key + key
    l.reproject_ref_frame.restype = C.c_int
    l.reproject_ref_frame.argtypes = [C.POINTER(RtHipScene), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(RtHipTemporalParams), C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]
    return l


def params(**fields) -> RtHipTemporalParams:
    """The defaults (default_temporal_params of rt_amd/csrc/temporal.cpp) with `fields` replaced."""
    p = RtHipTemporalParams()
    lib().reproject_ref_default_params(C.byref(p))
    for name, value in fields.items():
        assert hasattr(p, name), name
        setattr(p, name, value)
    return p


def check(p: RtHipTemporalParams):
    """check_temporal_params: (status, message)."""
    message = C.create_string_buffer(256)
    status = lib().reproject_ref_check(C.byref(p), message, len(message))
    return status, message.value.decode()


def forward(inverse):
    """forward_view_projection: (status, float32[4, 4] or None, message)."""
    inverse = np.ascontiguousarray(inverse, dtype=F32).reshape(16)
    out = np.full(16, np.nan, dtype=F32)
    message = C.create_string_buffer(256)
    status = lib().reproject_ref_forward(inverse.ctypes.data, out.ctypes.data, message, len(message))
    return status, (out.reshape(4, 4) if status == 0 else None), message.value.decode()


KEY_FIELDS = ("scene_fingerprint", "samples_per_pixel", "max_bounces", "matrix", "width", "height", "seed", "flags")


def same_history(a: dict, b: dict) -> bool:
    """same_history on two frame keys given as dictionaries of KEY_FIELDS."""
    args, keep = [], []
    for key in (a, b):
        assert set(key) == set(KEY_FIELDS)
        matrix = np.ascontiguousarray(key["matrix"], dtype=F32).reshape(16)
        keep.append(matrix)
        args += [key["scene_fingerprint"], key["samples_per_pixel"], key["max_bounces"], matrix.ctypes.data, key["width"], key["height"], key["seed"], key["flags"]]
    return bool(lib().reproject_ref_same_history(*args))


def matrix_of(scene: RtHipScene) -> np.ndarray:
    return np.array(list(scene.inverse_view_projection), dtype=F32)


def frame(scene: RtHipScene, guide: np.ndarray, rgb: np.ndarray, samples_in: int, prev_matrix=None, prev_rgb=None, prev_record=None, p: RtHipTemporalParams | None = None):
    """One step, serially — rt_hip_reproject_device's arguments on host arrays; `scene` stands for the resident scene (its matrix is
    the current camera).  Returns (rgb float32[H, W, 3], record float32[H, W, 8] with the id's bits in word 7, pixels with history)."""
    guide = np.ascontiguousarray(guide, dtype=F32)
    rgb = np.ascontiguousarray(rgb, dtype=F32)
    height, width = rgb.shape[:2]
    assert rgb.shape == (height, width, 3) and guide.shape == (height, width, 8)
    assert (prev_rgb is None) == (prev_record is None)
    if prev_rgb is not None:
        prev_rgb = np.ascontiguousarray(prev_rgb, dtype=F32)
        prev_record = np.ascontiguousarray(prev_record, dtype=F32)
        prev_matrix = np.ascontiguousarray(prev_matrix, dtype=F32).reshape(16)
        assert prev_rgb.shape == rgb.shape and prev_record.shape == guide.shape
    out = np.empty_like(rgb)
    record = np.empty((height, width, 8), dtype=F32)
    found = C.c_uint32()
    status = lib().reproject_ref_frame(C.byref(scene), width, height, prev_matrix.ctypes.data if prev_rgb is not None else None, guide.ctypes.data, rgb.ctypes.data, samples_in,
                                       prev_rgb.ctypes.data if prev_rgb is not None else None, prev_record.ctypes.data if prev_rgb is not None else None, C.byref(p) if p is not None else None, out.ctypes.data, record.ctypes.data, C.byref(found))
    if status != 0:
        raise ValueError(f"reproject_ref_frame refused its arguments ({status})")
    return out, record, found.value


def ids_of(record_or_guide: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(record_or_guide[..., 7]).view(np.uint32)


def sequence(frames, p: RtHipTemporalParams | None = None):
    """What rt_hip_render_temporal keeps and delivers (without the spatial filter) over `frames`, a list of (scene, guide, rgb,
    samples_in): a list of (blended rgb, record, pixels with history), each step's history being the step before."""
    out = []
    prev = None
    for scene, guide, rgb, samples_in in frames:
        if prev is None:
            step = frame(scene, guide, rgb, samples_in, p=p)
        else:
            step = frame(scene, guide, rgb, samples_in, prev[0], prev[1], prev[2], p)
        out.append(step)
        prev = (matrix_of(scene), step[0], step[1])
    return out
