"""ctypes binding of tests/native/libdenoise_reference.so — the CPU restatement of the guide-buffer denoiser: the serial
filter over rt_amd/csrc/denoise_rules.hpp with the oracle's leaf functions, `finish`, and rt_amd/csrc/denoise.cpp's parameter check.
TEST INFRASTRUCTURE.

Also here, shared by the CPU and the GPU tests: the yardstick of the GUIDE, composed in Python from what exists — the oracle's
centre ray of every pixel (oracle_primary_ray at 2^23, 2^23), its closest hit (box_reference's under the box flag) and the scene's
material columns.  No new C++ stands behind it."""
from __future__ import annotations

import ctypes as C
import functools
import subprocess

import numpy as np

from oracle import binding as oracle
from rt_amd.capi import RtHipDenoiseParams, RtHipScene
from tests import box_reference
from tests.conftest import ROOT

LIBRARY = ROOT / "tests" / "native" / "libdenoise_reference.so"
F32 = np.float32


@functools.lru_cache(maxsize=None)
def lib() -> C.CDLL:
    if not LIBRARY.exists():  # (`make` builds it with everything else; a tree that was never built gets it here)
        subprocess.run(["make", "-C", str(ROOT), str(LIBRARY.relative_to(ROOT))], check=True, capture_output=True)
    l = C.CDLL(str(LIBRARY))
    l.denoise_ref_default_params.restype = None
    l.denoise_ref_default_params.argtypes = [C.POINTER(RtHipDenoiseParams)]
    l.denoise_ref_check.restype = C.c_int
    l.denoise_ref_check.argtypes = [C.POINTER(RtHipDenoiseParams), C.c_char_p, C.c_size_t]
    l.denoise_ref_finish.restype = None
    l.denoise_ref_finish.argtypes = [C.c_size_t, C.c_void_p, C.c_void_p]
    l.denoise_ref_filter.restype = C.c_int
    l.denoise_ref_filter.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(RtHipDenoiseParams), C.c_void_p, C.c_void_p]
    return l


def params(**fields) -> RtHipDenoiseParams:
    """The defaults (default_denoise_params of rt_amd/csrc/denoise.cpp) with `fields` replaced."""
    p = RtHipDenoiseParams()
    lib().denoise_ref_default_params(C.byref(p))
    for name, value in fields.items():
        assert hasattr(p, name), name
        setattr(p, name, value)
    return p


def check(p: RtHipDenoiseParams):
    """check_denoise_params: (status, message)."""
    message = C.create_string_buffer(256)
    status = lib().denoise_ref_check(C.byref(p), message, len(message))
    return status, message.value.decode()


def finish(rgb: np.ndarray) -> np.ndarray:
    """finish(): float32[..., 3] means -> uint32[...] packed pixels."""
    rgb = np.ascontiguousarray(rgb, dtype=F32)
    out = np.empty(rgb.shape[:-1], dtype=np.uint32)
    lib().denoise_ref_finish(out.size, rgb.ctypes.data, out.ctypes.data)
    return out


def filter(rgb: np.ndarray, guide: np.ndarray, p: RtHipDenoiseParams | None = None):
    """The whole filter, serially: rgb float32[H, W, 3], guide float32[H, W, 8] -> (rgb float32[H, W, 3], rgba uint32[H, W])."""
    rgb = np.ascontiguousarray(rgb, dtype=F32)
    guide = np.ascontiguousarray(guide, dtype=F32)
    height, width = rgb.shape[:2]
    assert rgb.shape == (height, width, 3) and guide.shape == (height, width, 8)
    out = np.empty_like(rgb)
    rgba = np.empty((height, width), dtype=np.uint32)
    status = lib().denoise_ref_filter(width, height, rgb.ctypes.data, guide.ctypes.data, C.byref(p) if p is not None else None, out.ctypes.data, rgba.ctypes.data)
    if status != 0:
        raise ValueError(f"denoise_ref_filter refused the parameters ({status}): {check(p)[1]}")
    return out, rgba


def _column(pointer, n, dtype):
    return np.ctypeslib.as_array(pointer, shape=(n,)).astype(dtype) if n else np.zeros(0, dtype=dtype)


def compose_guide(scene: RtHipScene, width: int, height: int, boxes: bool = False) -> np.ndarray:
    """The guide of `scene` as the oracle sees it, float32[H, W, 8] (word 7 holds the id's bits): per pixel the centre ray, its closest
    hit (`boxes`: with the scene's boxes, tests/native/box_reference.cpp), then normal, depth | attenuation or sky, id."""
    origins = np.empty((height, width, 3), dtype=F32)
    directions = np.empty((height, width, 3), dtype=F32)
    for y in range(height):
        for x in range(width):
            origins[y, x], directions[y, x] = oracle.primary_ray(scene, width, height, x, y, 2.0**23, 2.0**23)
    hit = box_reference.closest_hit if boxes else oracle.closest_hit
    distance, kind, index, normal = hit(scene, origins.reshape(-1, 3), directions.reshape(-1, 3))
    n_materials = scene.n_materials
    albedo = _column(scene.material_albedo, n_materials * 4, F32).reshape(-1, 4)
    reflectivity = _column(scene.material_reflectivity, n_materials, F32)
    attenuation = (albedo[:, :3] * reflectivity[:, None]).astype(F32)  # one float multiply per channel (mg_ray_tracer.cpp:115)
    material_of = [None, _column(scene.sphere_material, scene.n_spheres, np.uint32), _column(scene.plane_material, scene.n_planes, np.uint32), _column(scene.box_material, scene.n_boxes, np.uint32)]
    first_of = [0, 0, scene.n_spheres, scene.n_spheres + scene.n_planes]
    guide = np.zeros((height * width, 8), dtype=F32)
    ids = np.zeros(height * width, dtype=np.uint32)
    flat_directions = directions.reshape(-1, 3)
    for i in range(height * width):
        k = int(kind[i])
        if k == 0:
            guide[i, 3] = -1.0
            guide[i, 4:7] = oracle.sky(float(flat_directions[i, 1]))
        else:
            assert k in (1, 2) or (boxes and k == 3)
            guide[i, 0:3] = normal[i]
            guide[i, 3] = distance[i]
            guide[i, 4:7] = attenuation[material_of[k][index[i]]]
            ids[i] = 1 + first_of[k] + int(index[i])
    guide[:, 7] = ids.view(F32)
    return guide.reshape(height, width, 8)
