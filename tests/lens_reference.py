"""ctypes binding of tests/native/liblens_reference.so — the CPU restatement of RT_HIP_FLAG_THIN_LENS: the frozen oracle
with a sample loop that knows a lens, over rt_amd/csrc/lens_rules.hpp (the text the device runs) and rt_amd/csrc/lens.cpp as it is.  TEST
INFRASTRUCTURE.  `render` has the call shape of oracle.binding's plus the lens; with no lens or a radius of 0 it is the oracle's, bit for
bit (tests/test_lens_reference.py).

Also here, shared by the CPU and the GPU tests: the numerator lattice and its edge words, the three cameras and scenes of our own
primitives."""
from __future__ import annotations

import ctypes as C
import functools
import subprocess

import numpy as np

import rt_amd
from oracle import binding as oracle
from oracle.binding import OracleStats
from rt_amd.capi import RtHipLens, RtHipPartition, RtHipScene
from tests.conftest import ROOT

LIBRARY = ROOT / "tests" / "native" / "liblens_reference.so"

# the three cameras of the GPU tests: rt's axis-aligned one (a pinhole in binary32), a tilted one (the plain eye form) and the matrix the
# parity tests use to reach the guarded eye form (tests/test_gpu_parity.py: the tilted matrix with its depth column scaled)
AXIS_CAMERA = ((0.0, 1.0, 3.0), (0.0, 0.0, -1.0))
TILTED_CAMERA = ((0.3, 1.5, 5.0), (0.2, -0.15, -1.0))


@functools.lru_cache(maxsize=None)
def lib() -> C.CDLL:
    if not LIBRARY.exists():  # (`make` builds it with everything else; a tree that was never built gets it here)
        subprocess.run(["make", "-C", str(ROOT), str(LIBRARY.relative_to(ROOT))], check=True, capture_output=True)
    l = C.CDLL(str(LIBRARY))
    l.lens_ref_render.restype = C.c_int
    l.lens_ref_render.argtypes = [C.POINTER(RtHipScene), C.c_uint32, C.c_uint32, C.c_uint64, C.c_int, C.POINTER(RtHipPartition), C.c_void_p, C.c_void_p, C.c_int, C.POINTER(OracleStats), C.POINTER(RtHipLens)]
    l.lens_ref_ray.restype = C.c_int
    l.lens_ref_ray.argtypes = [C.POINTER(RtHipScene), C.c_uint32, C.c_uint32, C.c_uint64, C.POINTER(RtHipLens), C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]
    l.lens_ref_disk.restype = None
    l.lens_ref_disk.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    l.lens_ref_bend.restype = None
    l.lens_ref_bend.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    l.lens_ref_words.restype = C.c_int
    l.lens_ref_words.argtypes = [C.POINTER(RtHipScene), C.c_uint32, C.c_uint32, C.POINTER(RtHipLens), C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]
    l.lens_ref_check_lens.restype = C.c_int
    l.lens_ref_check_lens.argtypes = [C.c_float, C.c_float, C.c_char_p, C.c_size_t]
    l.lens_ref_from_spec.restype = C.c_int
    l.lens_ref_from_spec.argtypes = [C.c_char_p, C.POINTER(RtHipLens), C.c_char_p, C.c_size_t]
    l.lens_ref_check_frame.restype = C.c_int
    l.lens_ref_check_frame.argtypes = [C.POINTER(RtHipScene), C.c_uint32, C.c_uint32, C.c_int, C.c_char_p, C.c_size_t]
    return l


def lens_of(lens):
    """None, an RtHipLens or (aperture_radius, focus_distance)."""
    if lens is None or isinstance(lens, RtHipLens):
        return lens
    return RtHipLens(*lens)


def render(scene: RtHipScene, width: int, height: int, lens=None, seed: int = 1, partition=None, want_rgb=True, threads: int = 0, sm_materials: bool = False):
    """lens_ref_render: (rgba uint32[rows, W], rgb float32[rows, W, 3] | None, stats dict), as oracle.binding.render returns them."""
    rows = height if partition is None else sum(1 for y in range(height) if (y // partition[2]) % partition[1] == partition[0])
    rgba = np.zeros((rows, width), dtype=np.uint32)
    rgb = np.zeros((rows, width, 3), dtype=np.float32) if want_rgb else None
    stats = OracleStats()
    part = C.byref(RtHipPartition(*partition)) if partition is not None else None
    the_lens = lens_of(lens)
    rc = lib().lens_ref_render(C.byref(scene), width, height, seed, oracle.MATERIALS_SM if sm_materials else 0, part, rgba.ctypes.data, rgb.ctypes.data if rgb is not None else None, threads or oracle.default_threads(), C.byref(stats),
                               C.byref(the_lens) if the_lens is not None else None)
    if rc != 0:
        raise RuntimeError(f"lens_ref_render failed ({rc})")
    return rgba, rgb, stats.as_dict()


def ray(scene: RtHipScene, width: int, height: int, lens, x: int, y: int, sample: int, seed: int = 1):
    """lens_ref_ray: (ray float32[6], pinhole ray float32[6], numerators uint32[4] = jitter ka, kb, lens ka, kb; steps drawn before the trace)."""
    out, pinhole, numerators, steps = np.zeros(6, dtype=np.float32), np.zeros(6, dtype=np.float32), np.zeros(4, dtype=np.uint32), C.c_uint32(0)
    the_lens = lens_of(lens)
    rc = lib().lens_ref_ray(C.byref(scene), width, height, seed, C.byref(the_lens) if the_lens is not None else None, x, y, sample, out.ctypes.data, pinhole.ctypes.data, numerators.ctypes.data, C.byref(steps))
    if rc != 0:
        raise RuntimeError(f"lens_ref_ray failed ({rc})")
    return out, pinhole, numerators, steps.value


def disk(ka: np.ndarray, kb: np.ndarray) -> np.ndarray:
    """lens_ref_disk: float32[n, 2]."""
    ka, kb = np.ascontiguousarray(ka, dtype=np.uint32), np.ascontiguousarray(kb, dtype=np.uint32)
    out = np.zeros((len(ka), 2), dtype=np.float32)
    lib().lens_ref_disk(len(ka), ka.ctypes.data, kb.ctypes.data, out.ctypes.data)
    return out


def bend(ka, kb, ray_words, lens_words) -> np.ndarray:
    """lens_ref_bend: float32[n, 9] = (lx, ly, origin, direction, bent), what rt_hip_kat_lens computes on the device."""
    ka, kb = np.ascontiguousarray(ka, dtype=np.uint32), np.ascontiguousarray(kb, dtype=np.uint32)
    ray_words, lens_words = np.ascontiguousarray(ray_words, dtype=np.float32), np.ascontiguousarray(lens_words, dtype=np.float32)
    assert ray_words.shape == (9,) and lens_words.shape == (10,)
    out = np.zeros((len(ka), 9), dtype=np.float32)
    lib().lens_ref_bend(len(ka), ka.ctypes.data, kb.ctypes.data, ray_words.ctypes.data, lens_words.ctypes.data, out.ctypes.data)
    return out


def words(scene: RtHipScene, width: int, height: int, lens):
    """lens_ref_words: (status, words float32[10] = U, V, fwd, focus; eye float32[3]; form 1 pinhole, 2 plain eye, 3 guarded eye)."""
    out, eye, form = np.zeros(10, dtype=np.float32), np.zeros(3, dtype=np.float32), C.c_uint32(0)
    the_lens = lens_of(lens)
    status = lib().lens_ref_words(C.byref(scene), width, height, C.byref(the_lens), out.ctypes.data, eye.ctypes.data, C.byref(form))
    return status, out, eye, form.value


def check_lens(aperture_radius: float, focus_distance: float):
    message = C.create_string_buffer(256)
    status = lib().lens_ref_check_lens(aperture_radius, focus_distance, message, 256)
    return status, message.value.decode()


def from_spec(spec):
    """(status, message, RtHipLens): the lens is the sentinel (-1, -1) where the parser left it alone."""
    message, lens = C.create_string_buffer(256), RtHipLens(-1.0, -1.0)
    status = lib().lens_ref_from_spec(spec.encode() if isinstance(spec, str) else spec, C.byref(lens), message, 256)
    return status, message.value.decode(), lens


def check_frame(scene: RtHipScene, width: int, height: int, have_lens: bool):
    message = C.create_string_buffer(256)
    status = lib().lens_ref_check_frame(C.byref(scene), width, height, int(have_lens), message, 256)
    return status, message.value.decode()


# ---- the numerator lattice of the rules tests (CPU and device): 2^16 x 16 pairs and the edge words ---------------------------------
TOP = (1 << 24) - 1
HALF = 1 << 23
EDGE_WORDS = [(0, 0), (TOP, TOP), (HALF, HALF),  # both 0, both 2^24 - 1, both 2^23 (the zero point)
              (HALF + 4096, HALF + 4096), (HALF + 4096, HALF - 4096),  # the two ties |x| == |y|
              (HALF + 1, HALF), (HALF - 1, HALF), (HALF, HALF + 1), (HALF, HALF - 1), (HALF + 1, HALF + 1), (HALF - 1, HALF - 1), (HALF + 1, HALF - 1),  # 2^23 +- 1
              (0, TOP), (TOP, 0), (0, HALF), (HALF, 0), (TOP, HALF), (HALF, TOP)]


def lattice():
    """(ka, kb) uint32[2^20 + edges]: a fixed rank-1 lattice over the 24-bit square — index i -> (i * 16 + 7, (i * 0x9E3779B1) >> 8) —
    whose points are equidistributed in both coordinates, followed by the edge words."""
    i = np.arange(1 << 20, dtype=np.uint64)
    ka = ((i * 16 + 7) & TOP).astype(np.uint32)
    kb = (((i * 0x9E3779B1) & 0xFFFFFFFF) >> 8).astype(np.uint32)
    edges = np.array(EDGE_WORDS, dtype=np.uint32)
    return np.concatenate([ka, edges[:, 0]]), np.concatenate([kb, edges[:, 1]])


# ---- scenes ---------------------------------------------------------------------------------------------------------------------
def named_scene(name: str, camera=None, spp=20, bounces=0):
    scene = rt_amd.Scene.named(name).set_sampling(spp, bounces)
    if camera is not None:
        scene.set_camera(*camera)
    return scene


def guarded(pod):
    """the parity tests' matrix for the guarded eye form: w depends on x and y (tests/test_gpu_parity.py)"""
    m = np.array(pod.inverse_view_projection[:], dtype=np.float32).reshape(4, 4)
    m[3, 0], m[3, 1] = 3.0, -2.0
    pod.inverse_view_projection = (C.c_float * 16)(*m.reshape(-1))
    return pod


def guarded_squarely(pod):
    """A guarded-eye matrix whose rays meet the focus plane as squarely as the camera's own: every entry times 2^-52.  The un-projected
    points are the same points (a homogeneous matrix has no scale), but s N.w lies below the 2^-50 the plain eye form asks for
    (frame_setup.cpp), so the frame takes the guarded reciprocal."""
    m = np.array(pod.inverse_view_projection[:], dtype=np.float32) * np.float32(2.0**-52)
    pod.inverse_view_projection = (C.c_float * 16)(*m)
    return pod


FORM_OF = {"pinhole": 1, "eye": 2, "guarded": 3}  # (what lens_ref_words reports)


def camera_pod(name, form, width=64, height=36, spp=20, bounces=0):
    """the named scene through the camera that reaches `form`: rt's axis-aligned one, a tilted one, the guarded-eye matrix"""
    if form == "pinhole":
        pod = named_scene(name, AXIS_CAMERA, spp, bounces).describe(width, height)
    elif form == "eye":
        pod = named_scene(name, TILTED_CAMERA, spp, bounces).describe(width, height)
    else:
        pod = guarded(named_scene(name, None, spp, bounces).describe(width, height))
    assert oracle.primary_ray(pod, width, height, 0, 0, want_form=True)[2] == ("eye" if form == "guarded" else form)
    assert words(pod, width, height, (0.06, 3.4))[3] == FORM_OF[form]
    return pod


# material types of include/rt_hip.h, as the scenes below use them
LAMBERT, METAL, DIELECTRIC = 0, 1, 2
MATERIALS = [(LAMBERT, (0.8, 0.8, 0.3), 0.0, 1.0), (METAL, (0.9, 0.6, 0.4), 0.2, 0.9), (DIELECTRIC, (0.9, 0.95, 1.0), 0.0, 1.5), (LAMBERT, (0.3, 0.5, 0.8), 0.0, 0.8)]


def scene_pod(camera: RtHipScene, spheres=(), planes=(), spp=20, bounces=6, materials=MATERIALS, matrix=None) -> RtHipScene:
    """An rt_hip_scene of our own primitives seen through `camera`'s matrix (any pod described for the frame's size) or `matrix`.
    spheres: (x, y, z, r, material); planes: (nx, ny, nz, d, material); materials: (type, albedo rgb, roughness, reflectivity)."""
    from rt_amd.scene import scene_from_arrays

    rows = [(kind, *albedo, 1.0, roughness, reflectivity) for kind, albedo, roughness, reflectivity in materials]
    if matrix is None:
        matrix = np.array(list(camera.inverse_view_projection), dtype=np.float32).reshape(4, 4)
    return scene_from_arrays(spheres=list(spheres) or None, planes=list(planes) or None, materials=rows, samples_per_pixel=spp, max_bounces=bounces, inverse_view_projection=np.asarray(matrix, dtype=np.float32).reshape(4, 4))


def grid_spheres(count, radius=0.12, pitch=0.3, material_count=4):
    side = int(np.ceil(np.sqrt(count)))
    return [((i % side - side / 2) * pitch, radius, -(i // side) * pitch, radius, i % material_count) for i in range(count)]
