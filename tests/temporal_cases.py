"""Scenes, cameras and moves shared by the tests of temporal accumulation (tests/test_reproject_reference.py on the CPU,
tests/test_gpu_temporal.py on the device).  TEST INFRASTRUCTURE: everything is composed from the oracle and the CPU restatements and
cached, so that a yardstick is computed once and never changed."""
from __future__ import annotations

import functools

import numpy as np

import rt_amd
from oracle import binding as oracle
from tests import box_reference as box_ref
from tests import denoise_reference as guide_ref
from tests import reproject_reference as ref
from tests.conftest import GOLDEN

F32 = np.float32
FORWARD = (0.0, 0.0, -1.0)
EYE = (0.0, 1.0, 3.0)  # basic.toml's camera
TILTED = ((0.2, 1.2, 3.0), (0.0, -0.15, -1.0))  # an eye-form matrix (tests/test_gpu_denoise.py)
# primitives in front of AND behind basic.toml's camera, for the turns by 180 degrees: (x, y, z, r, material), (nx, ny, nz, d, material)
SURROUND_SPHERES = [(0, 1, 0, 1, 0), (2, 0.5, -1, 0.5, 1), (-1.5, 0.4, 1, 0.4, 3), (0.5, 1, 6.5, 1, 1), (-2, 0.8, 7, 0.8, 3)]
SURROUND_PLANES = [(0, 1, 0, 0, 0)]


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def yaw(direction, degrees):
    """`direction` turned about the y axis."""
    a = np.radians(degrees)
    x, y, z = direction
    return (float(x * np.cos(a) + z * np.sin(a)), float(y), float(-x * np.sin(a) + z * np.cos(a)))


def toml_scene(name, width, height, position=None, direction=None, spp=16):
    """scenes/<name>.toml (boxes: the golden scene) seen from `position` along `direction` (None: the file's own camera)."""
    scene = rt_amd.Scene.load(GOLDEN / "scenes" / "boxes.toml") if name == "boxes" else rt_amd.Scene.named(name)
    if position is not None:
        scene.set_camera(position, direction if direction is not None else FORWARD)
    return scene.set_sampling(spp).describe(width, height)


def surround(width, height, position=EYE, direction=FORWARD, spp=16):
    """SURROUND_* through the matrix of a camera at `position` looking along `direction`."""
    return box_ref.scene_pod(toml_scene("basic", width, height, position, direction), spheres=SURROUND_SPHERES, planes=SURROUND_PLANES, spp=spp)


ORTHOGRAPHIC = np.array([[4, 0, 0, 0.25], [0, 2.25, 0.5, 1.5], [0, 0, -10, 5], [0, 0, 0, 1]], dtype=F32)  # no finite eye: the homogeneous form
ABOUT_FACE = np.array([[-1, 0, 0, 0.5], [0, 1, 0, 0], [0, 0, -1, 10], [0, 0, 0, 1]], dtype=F32)  # half a turn about the vertical through (0.25, ., 5)


def with_matrix(pod, matrix):
    """`pod`'s primitives through `matrix` (float32[4, 4], clip -> world)."""
    out = box_ref.scene_pod(pod, spheres=SURROUND_SPHERES, planes=SURROUND_PLANES, spp=pod.samples_per_pixel)
    for i, v in enumerate(np.asarray(matrix, dtype=F32).reshape(-1)):
        out.inverse_view_projection[i] = float(v)
    return out


def orthographic(width, height, turned=False, shift=0.0):
    matrix = (ABOUT_FACE @ ORTHOGRAPHIC if turned else ORTHOGRAPHIC).astype(F32)
    matrix[0, 3] += shift
    return with_matrix(toml_scene("basic", width, height), matrix)


def guarded(width, height, position=EYE, direction=FORWARD):
    """basic.toml through a perspective matrix whose w changes sign inside the frame: the eye form with its guarded reciprocal and the
    direction flip (tests/test_gpu_parity.py)."""
    pod = toml_scene("basic", width, height, position, direction)
    matrix = ref.matrix_of(pod).reshape(4, 4)
    matrix[3, 0], matrix[3, 1] = 3.0, -2.0
    for i, v in enumerate(matrix.reshape(-1)):
        pod.inverse_view_projection[i] = float(v)
    return pod


def planes_and_sky(width, height, position=EYE):
    """A floor and a slope that rises to the left, nothing else: the upper right of the frame is sky."""
    return box_ref.scene_pod(toml_scene("basic", width, height, position, FORWARD), planes=[(0, 1, 0, 0, 0), (0.6, 0.8, 0, 2, 3)], spp=16)


def guide_of(pod, width, height, boxes=False):
    return guide_ref.compose_guide(pod, width, height, boxes=boxes)


def oracle_mean(pod, width, height, seed, boxes=False):
    return (box_ref.render if boxes else oracle.render)(pod, width, height, seed=seed)[1]


def ramp(width, height):
    """A colour that encodes each pixel's own coordinates: r = x, g = y, b = 1."""
    image = np.ones((height, width, 3), dtype=F32)
    image[..., 0], image[..., 1] = np.arange(width, dtype=F32)[None, :], np.arange(height, dtype=F32)[:, None]
    return image


# ---- the cases the device is held to, by name: (width, height, [pods of the frames in order], boxes) --------------------------
def _moves(make, width, height):
    """rest, dolly, yaw, about-face: lists of two pods (previous, current)."""
    position, direction = make
    return {
        "rest": [(position, direction), (position, direction)],
        "dolly": [(position, direction), ((position[0] + 0.11, position[1] + 0.02, position[2] - 0.07), direction)],
        "yaw": [(position, direction), (position, yaw(direction, 4.0))],
        "about_face": [(position, direction), (position, yaw(direction, 180.0))],
    }


@functools.lru_cache(maxsize=None)
def case(name, width, height):
    """-> (pods, guides, boxes): two frames of a move, the guide of each (read-only)."""
    scene, _, move = name.partition(":")
    boxes = scene == "boxes"
    if scene == "orthographic":
        pods = {"rest": [orthographic(width, height), orthographic(width, height)], "dolly": [orthographic(width, height), orthographic(width, height, shift=0.3)],
                "about_face": [orthographic(width, height), orthographic(width, height, turned=True)]}[move]
    else:
        start = {"basic": (EYE, FORWARD), "tilted": TILTED, "surround": (EYE, FORWARD), "surround_tilted": TILTED, "planes_and_sky": (EYE, FORWARD), "boxes": ((0.5, 1.6, 5.5), (0.0, -0.2, -1.0)), "basic_plane": (EYE, FORWARD), "guarded": (EYE, FORWARD)}[scene]
        cameras = _moves(start, width, height)[move]
        if scene in ("surround", "surround_tilted"):
            pods = [surround(width, height, *c) for c in cameras]
        elif scene == "guarded":
            pods = [guarded(width, height, *c) for c in cameras]
        elif scene == "planes_and_sky":
            pods = [box_ref.scene_pod(toml_scene("basic", width, height, *c), planes=[(0, 1, 0, 0, 0), (0.6, 0.8, 0, 2, 3)], spp=16) for c in cameras]
        else:
            pods = [toml_scene({"tilted": "basic"}.get(scene, scene), width, height, *c) for c in cameras]
    guides = [guide_of(pod, width, height, boxes) for pod in pods]
    for guide in guides:
        guide.setflags(write=False)
    return pods, guides, boxes


def first_history(name, width, height, samples=16, seed=3):
    """The history a first frame leaves: (matrix, rgb, record) of frame 0 of `case(name)` blended with nothing, from its oracle mean."""
    pods, guides, boxes = case(name, width, height)
    rgb, record, _ = ref.frame(pods[0], guides[0], oracle_mean(pods[0], width, height, seed, boxes), samples)
    return ref.matrix_of(pods[0]), rgb, record
