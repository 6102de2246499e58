"""ctypes binding of tests/native/libdirect_reference.so — the CPU restatement of RT_HIP_FLAG_DIRECT_LIGHT: the frozen
oracle with light_reference.cpp's trace loop plus the vertex rule of rt_amd/csrc/direct_light_rules.hpp.  TEST INFRASTRUCTURE.
`render` has tests.light_reference.render's call shape plus `direct`; with no sampled light it is that function's frame bit for bit
(tests/test_direct_reference.py).  Shared by the CPU and the GPU tests."""
from __future__ import annotations

import ctypes as C
import functools
import subprocess

import numpy as np

from oracle import binding as oracle
from oracle.binding import OracleStats
from rt_amd.capi import RtHipPartition, RtHipScene
from tests.conftest import ROOT
from tests.light_reference import table_of

LIBRARY = ROOT / "tests" / "native" / "libdirect_reference.so"
MAX_SAMPLED_LIGHTS = 256
# the restatement's own events, in the order of direct_reference.cpp's own_event (direct_ref_render_census fills one count per name)
OWN_EVENTS = ["vertex_aimed", "vertex_not_aimed", "shadow_visible", "shadow_occluded", "zero_word_k", "fold_below", "inside_light", "sampled_light_after_sampling_vertex", "sampled_light_after_other_vertex",
              "light_on_primary", "chose_last_of_256", "first_vertex_aimed", "first_vertex_not_aimed", "sampled_light_after_other_vertex_later"]


@functools.lru_cache(maxsize=None)
def lib() -> C.CDLL:
    if not LIBRARY.exists():  # (`make` builds it with everything else; a tree that was never built gets it here)
        subprocess.run(["make", "-C", str(ROOT), str(LIBRARY.relative_to(ROOT))], check=True, capture_output=True)
    l = C.CDLL(str(LIBRARY))
    l.direct_ref_render.restype = C.c_int
    l.direct_ref_render.argtypes = [C.POINTER(RtHipScene), C.c_uint32, C.c_uint32, C.c_uint64, C.c_int, C.POINTER(RtHipPartition), C.c_void_p, C.c_void_p, C.c_int, C.POINTER(OracleStats), C.c_void_p, C.c_uint32, C.c_int]
    l.direct_ref_render_census.restype = C.c_int
    l.direct_ref_render_census.argtypes = l.direct_ref_render.argtypes + [C.c_void_p, C.c_void_p, C.c_int64, C.c_uint32, C.c_void_p]
    l.direct_ref_own_events.restype = C.c_int
    l.direct_ref_own_events.argtypes = []
    assert l.direct_ref_own_events() == len(OWN_EVENTS)
    l.direct_ref_count.restype = C.c_int
    l.direct_ref_count.argtypes = [C.POINTER(RtHipScene), C.c_void_p, C.c_uint32]
    l.direct_ref_vertex.restype = C.c_int
    l.direct_ref_vertex.argtypes = [C.POINTER(RtHipScene), C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_void_p]
    l.direct_ref_octahedral.restype = None
    l.direct_ref_octahedral.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p]
    l.direct_ref_aim.restype = None
    l.direct_ref_aim.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_float, C.c_uint32, C.c_void_p]
    return l


def render(scene: RtHipScene, width: int, height: int, emission=None, seed: int = 1, partition=None, want_rgb=True, threads: int = 0, sm_materials: bool = False, direct: bool = True):
    """direct_ref_render: (rgba uint32[rows, W], rgb float32[rows, W, 3] | None, stats dict), as tests.light_reference.render returns them."""
    rows = height if partition is None else sum(1 for y in range(height) if (y // partition[2]) % partition[1] == partition[0])
    rgba = np.zeros((rows, width), dtype=np.uint32)
    rgb = np.zeros((rows, width, 3), dtype=np.float32) if want_rgb else None
    stats = OracleStats()
    part = C.byref(RtHipPartition(*partition)) if partition is not None else None
    table = table_of(emission, scene.n_materials)
    rc = lib().direct_ref_render(C.byref(scene), width, height, seed, oracle.MATERIALS_SM if sm_materials else 0, part, rgba.ctypes.data, rgb.ctypes.data if rgb is not None else None, threads or oracle.default_threads(), C.byref(stats),
                                 table.ctypes.data, len(table), int(direct))
    if rc != 0:
        raise RuntimeError(f"direct_ref_render failed ({rc})")
    return rgba, rgb, stats.as_dict()


def render_census(scene: RtHipScene, width: int, height: int, emission=None, seed: int = 1, threads: int = 0, sm_materials: bool = False, direct: bool = True, rare_rules: bool = True, watch=None):
    """direct_ref_render_census: render()'s frame with both censuses — (rgba, rgb, stats dict, {oracle event: count}, {own event: count},
    {own event: count of the watched sample} | None).  `watch` is (pixel, sample): the one sample whose own events are counted apart.
    rare_rules=False is oracle.render_census's test-only mode (no re-draw of a zero vector, no approx_zero replacement) under this loop."""
    rgba = np.zeros((height, width), dtype=np.uint32)
    rgb = np.zeros((height, width, 3), dtype=np.float32)
    stats = OracleStats()
    table = table_of(emission, scene.n_materials)
    census = np.zeros(len(oracle.CENSUS_EVENTS), dtype=np.uint64)
    own = np.zeros(len(OWN_EVENTS), dtype=np.uint64)
    watched = np.zeros(len(OWN_EVENTS), dtype=np.uint64)
    mode = oracle.TRACE_ITERATIVE | (oracle.MATERIALS_SM if sm_materials else 0) | (0 if rare_rules else oracle.TEST_NO_RARE_RULES)
    rc = lib().direct_ref_render_census(C.byref(scene), width, height, seed, mode, None, rgba.ctypes.data, rgb.ctypes.data, threads or oracle.default_threads(), C.byref(stats), table.ctypes.data, len(table), int(direct),
                                        census.ctypes.data, own.ctypes.data, -1 if watch is None else watch[0], 0 if watch is None else watch[1], watched.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"direct_ref_render_census failed ({rc})")
    named = lambda names, counts: {name: int(n) for name, n in zip(names, counts)}
    return rgba, rgb, stats.as_dict(), named(oracle.CENSUS_EVENTS, census), named(OWN_EVENTS, own), None if watch is None else named(OWN_EVENTS, watched)


def count(scene: RtHipScene, emission) -> int:
    """how many sampled lights the scene has under the table"""
    table = table_of(emission, scene.n_materials)
    n = lib().direct_ref_count(C.byref(scene), table.ctypes.data, len(table))
    assert n >= 0
    return n


def vertex(scene: RtHipScene, emission, point, normal, draws: int, seed: int = 1, pixel: int = 0):
    """direct_ref_vertex: (mean weight, mean squared weight, shadow segments) of `draws` runs of the vertex rule at `point`."""
    table = table_of(emission, scene.n_materials)
    p = np.asarray(point, dtype=np.float32)
    n = np.asarray(normal, dtype=np.float32)
    out = np.zeros(3, dtype=np.float64)
    rc = lib().direct_ref_vertex(C.byref(scene), table.ctypes.data, len(table), p.ctypes.data, n.ctypes.data, seed, pixel, draws, out.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"direct_ref_vertex failed ({rc})")
    return float(out[0]), float(out[1]), int(out[2])


def octahedral(ka: int, kb: int) -> np.ndarray:
    """(x, y, z, l2) of the rules header's octahedral_point, as g++ compiles it"""
    out = np.zeros(4, dtype=np.float32)
    lib().direct_ref_octahedral(ka, kb, out.ctypes.data)
    return out


def aim(ka: int, kb: int, x, nrm, centre, radius: float, n: int) -> np.ndarray:
    """(w.xyz, weight, aimed) of the rules header's aim_at, as g++ compiles it"""
    vectors = np.concatenate([np.asarray(v, dtype=np.float32) for v in (x, nrm, centre)])
    out = np.zeros(5, dtype=np.float32)
    lib().direct_ref_aim(ka, kb, vectors.ctypes.data, np.float32(radius), n, out.ctypes.data)
    return out
