"""ctypes binding of tests/native/libbox_reference.so — the CPU restatement of RT_HIP_FLAG_TRACE_BOXES: the frozen
oracle with a test_boxes that hits.  TEST INFRASTRUCTURE.  `render` and `closest_hit` have the call shapes of oracle.binding's, so a
test can hand the same scene to both; with n_boxes == 0 they are the oracle's, bit for bit (tests/test_box_reference.py).

Also here, shared by the CPU and the GPU tests: scenes with boxes built straight into an ``rt_hip_scene`` (`scene_pod`) and the ray
set both sides answer (`known_answer_rays`)."""
from __future__ import annotations

import ctypes as C
import functools
import subprocess

import numpy as np

from oracle import binding as oracle
from oracle.binding import OracleStats
from rt_amd.capi import RtHipPartition, RtHipScene
from tests.conftest import ROOT

LIBRARY = ROOT / "tests" / "native" / "libbox_reference.so"
KIND_BOX = 3


@functools.lru_cache(maxsize=None)
def lib() -> C.CDLL:
    if not LIBRARY.exists():  # (`make` builds it with everything else; a tree that was never built gets it here)
        subprocess.run(["make", "-C", str(ROOT), str(LIBRARY.relative_to(ROOT))], check=True, capture_output=True)
    l = C.CDLL(str(LIBRARY))
    l.box_ref_render.restype = C.c_int
    l.box_ref_render.argtypes = [C.POINTER(RtHipScene), C.c_uint32, C.c_uint32, C.c_uint64, C.c_int, C.POINTER(RtHipPartition), C.c_void_p, C.c_void_p, C.c_int, C.POINTER(OracleStats)]
    l.box_ref_closest_hit.restype = None
    l.box_ref_closest_hit.argtypes = [C.POINTER(RtHipScene), C.c_uint32] + [C.c_void_p] * 6
    return l


def render(scene: RtHipScene, width: int, height: int, seed: int = 1, partition=None, want_rgb=True, threads: int = 0, sm_materials: bool = False):
    """box_ref_render: (rgba uint32[rows, W], rgb float32[rows, W, 3] | None, stats dict), as oracle.binding.render returns them."""
    rows = height if partition is None else sum(1 for y in range(height) if (y // partition[2]) % partition[1] == partition[0])
    rgba = np.zeros((rows, width), dtype=np.uint32)
    rgb = np.zeros((rows, width, 3), dtype=np.float32) if want_rgb else None
    stats = OracleStats()
    part = C.byref(RtHipPartition(*partition)) if partition is not None else None
    rc = lib().box_ref_render(C.byref(scene), width, height, seed, oracle.MATERIALS_SM if sm_materials else 0, part, rgba.ctypes.data, rgb.ctypes.data if rgb is not None else None, threads or oracle.default_threads(), C.byref(stats))
    if rc != 0:
        raise RuntimeError(f"box_ref_render failed ({rc})")
    return rgba, rgb, stats.as_dict()


def closest_hit(scene: RtHipScene, origins, directions):
    """box_ref_closest_hit: (distance, kind, index, normal); kind 3 = box."""
    o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(directions, dtype=np.float32).reshape(-1, 3)
    n = len(o)
    dist = np.empty(n, dtype=np.float32)
    kind = np.empty(n, dtype=np.uint32)
    index = np.empty(n, dtype=np.uint32)
    normal = np.empty((n, 3), dtype=np.float32)
    lib().box_ref_closest_hit(C.byref(scene), n, o.ctypes.data, d.ctypes.data, dist.ctypes.data, kind.ctypes.data, index.ctypes.data, normal.ctypes.data)
    return dist, kind, index, normal


# material types of include/rt_hip.h, as the scenes below use them
LAMBERT, METAL, DIELECTRIC = 0, 1, 2
MATERIALS = [(LAMBERT, (0.8, 0.8, 0.3), 0.0, 1.0), (METAL, (0.9, 0.6, 0.4), 0.2, 0.9), (DIELECTRIC, (0.9, 0.95, 1.0), 0.0, 1.5), (LAMBERT, (0.3, 0.5, 0.8), 0.0, 0.8)]


def scene_pod(camera: RtHipScene, spheres=(), planes=(), boxes=(), spp=20, bounces=6, materials=MATERIALS) -> RtHipScene:
    """An rt_hip_scene of our own primitives seen through `camera`'s matrix (any pod described for the frame's size).
    spheres: (x, y, z, r, material); planes: (nx, ny, nz, d, material); boxes: (cx, cy, cz, ex, ey, ez, material);
    materials: (type, albedo rgb, roughness, reflectivity)."""
    from rt_amd.scene import scene_from_arrays

    rows = [(kind, *albedo, 1.0, roughness, reflectivity) for kind, albedo, roughness, reflectivity in materials]
    return scene_from_arrays(spheres=list(spheres) or None, planes=list(planes) or None, materials=rows, boxes=list(boxes) or None, samples_per_pixel=spp, max_bounces=bounces,
                             inverse_view_projection=np.array(list(camera.inverse_view_projection), dtype=np.float32).reshape(4, 4))


# ---- the known-answer scene and rays (tests/test_box_reference.py by hand, tests/test_gpu_boxes.py against the device) ----
# box 0 and box 1 are identical (ties go to the lower index); box 2's top face lies in the plane y = 3 (plane 0), and sphere 0
# (centre (10, 2, 0), radius 1, inside box 2) touches that plane from below; box 3 is huge (the overflow case of the zero-component rule)
KAT_BOXES = [(0, 0, 0, 1, 2, 3, 0), (0, 0, 0, 1, 2, 3, 1), (10, 2, 0, 1, 1, 1, 2), (100, 0, 0, 1, 1, 3e38, 3)]
KAT_PLANES = [(0, -1, 0, 3, 0)]  # -y + 3 = 0
KAT_SPHERES = [(10, 2, 0, 1, 1)]


def known_answer_rays():
    """(origins, directions, expected) — expected[i] = (kind, index, t, normal) worked out by hand, or None where only the two
    implementations are compared."""
    inf, nan = float("inf"), float("nan")
    rows = []

    def ray(o, d, want):
        rows.append((o, d, want))

    # the six faces from outside: straight at each, from 5 away of the face
    ray((-6, 0, 0), (1, 0, 0), (3, 0, 5.0, (-1, 0, 0)))
    ray((6, 0, 0), (-1, 0, 0), (3, 0, 5.0, (1, 0, 0)))
    ray((0, -7, 0), (0, 1, 0), (3, 0, 5.0, (0, -1, 0)))
    ray((0, 2.5, 0), (0, -1, 0), (3, 0, 0.5, (0, 1, 0)))  # (from below the plane y = 3)
    ray((0, 0, -8), (0, 0, 1), (3, 0, 5.0, (0, 0, -1)))
    ray((0, 0, 8), (0, 0, -1), (3, 0, 5.0, (0, 0, 1)))
    # the six from inside: the exit face, its outward normal
    ray((0, 0, 0), (1, 0, 0), (3, 0, 1.0, (1, 0, 0)))
    ray((0, 0, 0), (-1, 0, 0), (3, 0, 1.0, (-1, 0, 0)))
    ray((0, 0, 0), (0, 1, 0), (3, 0, 2.0, (0, 1, 0)))
    ray((0, 0, 0), (0, -1, 0), (3, 0, 2.0, (0, -1, 0)))
    ray((0, 0, 0), (0, 0, 1), (3, 0, 3.0, (0, 0, 1)))
    ray((0, 0, 0), (0, 0, -1), (3, 0, 3.0, (0, 0, -1)))
    # parallel to two slabs, inside both (zeros of either sign) and outside one (a miss: the plane behind is not reached either)
    ray((-6, 0.5, -0.5), (1, 0.0, -0.0), (3, 0, 5.0, (-1, 0, 0)))
    ray((-6, -2.5, 0), (1, 0, 0), (0, 0, -1.0, (0, 0, 0)))
    # an exact edge hit: the x and y slabs are entered at the same t = 4 -> x, the first axis (a direction need not be normalised for
    # the query; with one that is, (0.6, 0.8, 0), nothing is exact in binary32 and only the two implementations are compared)
    ray((-5, -6, 0), (1, 1, 0), (3, 0, 4.0, (-1, 0, 0)))
    ray((-3.4, -5.2, 0), (0.6, 0.8, 0), None)
    ray((-5, 0, -7), (1, 0, 1), (3, 0, 4.0, (-1, 0, 0)))  # x and z together -> x
    ray((0, -6, -7), (0, 1, 1), (3, 0, 4.0, (0, -1, 0)))  # y and z together -> y
    # box 2's top face, plane 0 and sphere 0 (a = 3, disc = 1: t = 3 - 1) all at t = 2 from (10, 5, 0) straight down: the box wins
    ray((10, 5, 0), (0, -1, 0), (3, 2, 2.0, (0, 1, 0)))
    # a hit nearer than 0.001 is rejected and the far face (t = 2.0005) is NOT taken: from just outside the -x face of boxes 0 and 1,
    # on a line that meets nothing else
    ray((-1.0005, 1.5, 2), (1, 0, 0), (0, 0, -1.0, (0, 0, 0)))
    ray((-1.5, 1.5, 2), (1, 0, 0), (3, 0, 0.5, (-1, 0, 0)))
    # the sign of a zero component: inside the huge box 3, x and y slabs never left (far = +inf), z's exit distance overflows to
    # +inf too -> tmax = +inf, x is the first axis that equals it; its normal has the zero's sign bit
    ray((100, 0, -2e38), (0.0, 0.0, 1), (3, 3, inf, (1, 0, 0)))
    ray((100, 0, -2e38), (-0.0, 0.0, 1), (3, 3, inf, (-1, 0, 0)))
    # NaN: the origin on a slab's plane, parallel to it (0 * inf).  In x the NaN is dropped by the selects and the ray grazes
    # along the face; in z (the last select) it survives: a miss
    ray((1, 0, -8), (0.0, 0, 1), (3, 0, 5.0, (0, 0, -1)))
    ray((-6, 1.5, 3), (1, 0, 0.0), (0, 0, -1.0, (0, 0, 0)))
    # ... and what a dropped NaN takes with it: y = 2 is the top of boxes 0 and 1, which lie BEHIND this ray (x slab:
    # -9.9995 .. -7.9995).  In y, t2 = 0 * inf = NaN is the second operand of the axis' own selects and comes out of both; as the
    # second operand of the x-y select it then replaces x's distances, and as the first operand of the y-z select it is dropped:
    # tmin = -inf, tmax = +inf (z: inside, direction 0) -> a "hit" at +inf on z's exit face.  hits_box's arithmetic, as it stands.
    ray((8.9995, 2, 0), (1, 0, 0), (3, 0, inf, (0, 0, 1)))
    # a NaN direction component: every comparison fails
    ray((-6, 0, 0), (1, nan, 0), None)
    origins = np.array([r[0] for r in rows], dtype=np.float32)
    directions = np.array([r[1] for r in rows], dtype=np.float32)
    return origins, directions, [r[2] for r in rows]
