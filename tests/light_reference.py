"""ctypes binding of tests/native/liblight_reference.so — the CPU restatement of RT_HIP_FLAG_EMISSION: the frozen
oracle with a trace loop that knows lights.  TEST INFRASTRUCTURE.  `render` has the call shape of oracle.binding's plus the emission
table; with no light in the table it is the oracle's, bit for bit (tests/test_light_reference.py).

Also here, shared by the CPU and the GPU tests: the fixture scene (tests/golden/scenes/lights.toml), its table, scenes of our own
primitives (`scene_pod`) and the furnace."""
from __future__ import annotations

import ctypes as C
import functools
import subprocess

import numpy as np

import rt_amd
from oracle import binding as oracle
from oracle.binding import OracleStats
from rt_amd.capi import RtHipPartition, RtHipScene
from tests.conftest import GOLDEN, ROOT

LIBRARY = ROOT / "tests" / "native" / "liblight_reference.so"

# the fixture: material names of lights.toml in file order, and the table of the spec "lamp=4,3.2,2"
LIGHTS_TOML = GOLDEN / "scenes" / "lights.toml"
LIGHTS_NAMES = ["ground", "lamp", "clay", "brass", "glass"]
LIGHTS_SPEC = "lamp=4,3.2,2"
LIGHTS_TABLE = np.array([(0, 0, 0), (4, 3.2, 2), (0, 0, 0), (0, 0, 0), (0, 0, 0)], dtype=np.float32)


@functools.lru_cache(maxsize=None)
def lib() -> C.CDLL:
    if not LIBRARY.exists():  # (`make` builds it with everything else; a tree that was never built gets it here)
        subprocess.run(["make", "-C", str(ROOT), str(LIBRARY.relative_to(ROOT))], check=True, capture_output=True)
    l = C.CDLL(str(LIBRARY))
    l.light_ref_render.restype = C.c_int
    l.light_ref_render.argtypes = [C.POINTER(RtHipScene), C.c_uint32, C.c_uint32, C.c_uint64, C.c_int, C.POINTER(RtHipPartition), C.c_void_p, C.c_void_p, C.c_int, C.POINTER(OracleStats), C.c_void_p, C.c_uint32]
    return l


def table_of(emission, n_materials: int) -> np.ndarray:
    """float32[n_materials, 3]; None = no light."""
    if emission is None:
        return np.zeros((n_materials, 3), dtype=np.float32)
    table = np.ascontiguousarray(emission, dtype=np.float32).reshape(-1, 3)
    assert len(table) == n_materials, (len(table), n_materials)
    return table


def render(scene: RtHipScene, width: int, height: int, emission=None, seed: int = 1, partition=None, want_rgb=True, threads: int = 0, sm_materials: bool = False):
    """light_ref_render: (rgba uint32[rows, W], rgb float32[rows, W, 3] | None, stats dict), as oracle.binding.render returns them."""
    rows = height if partition is None else sum(1 for y in range(height) if (y // partition[2]) % partition[1] == partition[0])
    rgba = np.zeros((rows, width), dtype=np.uint32)
    rgb = np.zeros((rows, width, 3), dtype=np.float32) if want_rgb else None
    stats = OracleStats()
    part = C.byref(RtHipPartition(*partition)) if partition is not None else None
    table = table_of(emission, scene.n_materials)
    rc = lib().light_ref_render(C.byref(scene), width, height, seed, oracle.MATERIALS_SM if sm_materials else 0, part, rgba.ctypes.data, rgb.ctypes.data if rgb is not None else None, threads or oracle.default_threads(), C.byref(stats),
                                table.ctypes.data, len(table))
    if rc != 0:
        raise RuntimeError(f"light_ref_render failed ({rc})")
    return rgba, rgb, stats.as_dict()


def lights_scene(position=None, direction=None, spp=20, bounces=0):
    scene = rt_amd.Scene.load(LIGHTS_TOML).set_sampling(spp, bounces)
    if position is not None:
        scene.set_camera(position, direction)
    return scene


# material types of include/rt_hip.h, as the scenes below use them
LAMBERT, METAL, DIELECTRIC = 0, 1, 2
MATERIALS = [(LAMBERT, (0.8, 0.8, 0.3), 0.0, 1.0), (METAL, (0.9, 0.6, 0.4), 0.2, 0.9), (DIELECTRIC, (0.9, 0.95, 1.0), 0.0, 1.5), (LAMBERT, (0.3, 0.5, 0.8), 0.0, 0.8)]


def scene_pod(camera: RtHipScene, spheres=(), planes=(), spp=20, bounces=6, materials=MATERIALS) -> RtHipScene:
    """An rt_hip_scene of our own primitives seen through `camera`'s matrix (any pod described for the frame's size).
    spheres: (x, y, z, r, material); planes: (nx, ny, nz, d, material); materials: (type, albedo rgb, roughness, reflectivity)."""
    from rt_amd.scene import scene_from_arrays

    rows = [(kind, *albedo, 1.0, roughness, reflectivity) for kind, albedo, roughness, reflectivity in materials]
    return scene_from_arrays(spheres=list(spheres) or None, planes=list(planes) or None, materials=rows, samples_per_pixel=spp, max_bounces=bounces,
                             inverse_view_projection=np.array(list(camera.inverse_view_projection), dtype=np.float32).reshape(4, 4))


def grid_spheres(count, radius=0.12, pitch=0.3, material_count=4):
    side = int(np.ceil(np.sqrt(count)))
    return [((i % side - side / 2) * pitch, radius, -(i // side) * pitch, radius, i % material_count) for i in range(count)]


# ---- the furnace: the camera at the centre of ONE sphere whose material is a light -------------------------------------------------
FURNACE_E = (0.25, 0.5, 2.0)  # powers of two: a sum of equal powers of two is exact, so every pixel's float mean is exactly E


def furnace(width: int, height: int, spp: int):
    """(pod, table): basic.toml's camera (its eye at (0, 1, 3)) inside a sphere of radius 50 around the eye; one metal material
    (a light ignores its type)."""
    camera = rt_amd.Scene.named("basic").describe(width, height)
    pod = scene_pod(camera, spheres=[(0, 1, 3, 50, 0)], spp=spp, bounces=4, materials=[(METAL, (0.9, 0.6, 0.4), 0.3, 0.9)])
    return pod, np.array([FURNACE_E], dtype=np.float32)
