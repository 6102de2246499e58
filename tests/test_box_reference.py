"""The CPU restatement of RT_HIP_FLAG_TRACE_BOXES (tests/native/box_reference.cpp), held on three sides: to the frozen
oracle (without boxes it IS the oracle; a box hit's distance is oracle_hits_box's), to known answers worked out by hand from §3.7's
text, and to an independent binary64 slab test and face rule in numpy.  The GPU is held to the restatement in tests/test_gpu_boxes.py."""
import numpy as np
import pytest

import rt_amd
from oracle import binding as oracle
from tests import box_reference as box_ref
from tests.conftest import GOLDEN

SCENES_DIR = GOLDEN / "scenes"


def same_frame(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and a[2]["segments"] == b[2]["segments"]


@pytest.fixture(scope="module")
def oracle_frames():
    """oracle_render of the two reference scenes at 64x36x20, both tables, whole and as the three parts of a 3-way partition: computed once."""
    frames = {}
    for name in ("basic", "dielectric"):
        pod = rt_amd.Scene.named(name).set_sampling(20).describe(64, 36)
        for sm in (False, True):
            for part in (None, (0, 3, 8), (1, 3, 8), (2, 3, 8)):
                frames[name, sm, part] = oracle.render(pod, 64, 36, seed=5, sm_materials=sm, partition=part)
    return frames


@pytest.mark.parametrize("name", ["basic", "dielectric"])
@pytest.mark.parametrize("sm", [False, True])
def test_without_boxes_the_restatement_is_the_frozen_oracle(oracle_frames, name, sm):
    scene = rt_amd.Scene.named(name).set_sampling(20)
    pod = scene.describe(64, 36)
    assert pod.n_boxes == 0
    for part in (None, (0, 3, 8), (1, 3, 8), (2, 3, 8)):
        assert same_frame(box_ref.render(pod, 64, 36, seed=5, sm_materials=sm, partition=part), oracle_frames[name, sm, part]), (name, sm, part)


@pytest.mark.parametrize("name", ["basic", "dielectric"])
@pytest.mark.parametrize("sm", [False, True])
def test_a_box_wholly_behind_the_camera_changes_nothing(oracle_frames, name, sm):
    """A primary ray meets a box behind the camera at negative distances only: a miss.  Scattered rays do fly backwards, so the box
    also lies under the ground — inside the scenes' opaque ground sphere (centre (0, -1000, 0), radius 1000; lambert under both
    tables), whose surface every ray that heads for it hits first: tested by every query, never the answer."""
    scene = rt_amd.Scene.named(name).set_sampling(20)
    camera = scene.describe(64, 36)
    spheres = [(camera.sphere_center_x[i], camera.sphere_center_y[i], camera.sphere_center_z[i], camera.sphere_radius[i], camera.sphere_material[i]) for i in range(camera.n_spheres)]
    materials = [(camera.material_type[i], tuple(camera.material_albedo[4 * i + c] for c in range(3)), camera.material_roughness[i], camera.material_reflectivity[i]) for i in range(camera.n_materials)]
    assert spheres[0][:4] == (0.0, -1000.0, 0.0, 1000.0) and materials[spheres[0][4]][0] == box_ref.LAMBERT
    pod = box_ref.scene_pod(camera, spheres=spheres, boxes=[(0, -500, 400, 50, 50, 50, 0)], spp=20, bounces=camera.max_bounces, materials=materials)  # (z = 400: the cameras stand at z = 3 and 7 and look down -z)
    for part in (None, (0, 3, 8), (1, 3, 8), (2, 3, 8)):
        assert same_frame(box_ref.render(pod, 64, 36, seed=5, sm_materials=sm, partition=part), oracle_frames[name, sm, part]), (name, sm, part)


@pytest.fixture(scope="module")
def kat_scene():
    camera = rt_amd.Scene.named("basic").describe(64, 36)
    return box_ref.scene_pod(camera, box_ref.KAT_SPHERES, box_ref.KAT_PLANES, box_ref.KAT_BOXES)


def test_known_answers_by_hand(kat_scene):
    """The six faces from outside and from inside, a ray parallel to two slabs, exact edges (first axis in x, y, z order), identical
    boxes (lower index), a box face in a plane that a sphere touches at the same t (the box wins), a hit nearer than 0.001 (rejected,
    far face not taken), the sign of a zero component, the NaN cases: tests/box_reference.py has the rays and the derivations."""
    origins, directions, expected = box_ref.known_answer_rays()
    t, kind, index, normal = box_ref.closest_hit(kat_scene, origins, directions)
    checked = 0
    for i, want in enumerate(expected):
        if want is None:
            continue
        where = (i, tuple(origins[i]), tuple(directions[i]))
        assert (int(kind[i]), int(index[i])) == want[:2], where
        assert t[i] == np.float32(want[2]), where
        assert tuple(normal[i]) == tuple(np.float32(c) for c in want[3]), where
        checked += 1
    assert checked >= 24


def random_face_rays(rng, boxes, count):
    """Rays aimed at points of face interiors at least 1 % of the extent away from any edge, from origins outside the box (the face
    is entered) or inside it (the face is the exit): (origins, directions, box index, axis, sign, inside), all binary32 values."""
    rows = []
    for k in range(count):
        b = k % len(boxes)
        c, e = np.array(boxes[b][:3]), np.array(boxes[b][3:6])
        axis, sign, inside = int(rng.integers(3)), int(rng.choice([-1, 1])), bool(rng.integers(2))
        target = c + e * rng.uniform(-0.99, 0.99, 3)
        target[axis] = c[axis] + sign * e[axis]
        if inside:
            origin = c + e * rng.uniform(-0.9, 0.9, 3)
        else:  # in front of the face, within its outline: no other face is entered first
            origin = c + e * rng.uniform(-0.99, 0.99, 3)
            origin[axis] = c[axis] + sign * e[axis] * rng.uniform(1.5, 6.0)
        d = target - origin
        rows.append((origin, d / np.linalg.norm(d), b, axis, sign, inside))
    origins = np.array([r[0] for r in rows], dtype=np.float32)
    directions = np.array([r[1] for r in rows], dtype=np.float32)
    return origins, directions, rows


def slab_test_float64(o, d, c, e):
    """DESIGN.md §3.7 in binary64, written from its text: (hit, t, axis, sign)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / d
        t1, t2 = (c - e - o) * inv, (c + e - o) * inv
    near, far = np.minimum(t1, t2), np.maximum(t1, t2)
    tmin, tmax = near.max(), far.min()
    if not (tmax >= tmin) or tmax < 0:
        return False, -1.0, 0, 0
    if tmin >= 0:  # entering: the first axis whose near distance is tmin; the normal points against the direction's component
        axis = int(np.argmax(near == tmin))
        return True, tmin, axis, -1 if d[axis] > 0 else 1
    axis = int(np.argmax(far == tmax))  # leaving: the first axis whose far distance is tmax; the normal has the component's sign
    return True, tmax, axis, 1 if d[axis] > 0 else -1


def test_against_an_independent_float64_slab_test_and_face_rule():
    """10 000 random rays at face interiors, one box at a time (so that no other primitive decides): hit, face axis and sign equal,
    |t32 - t64| <= 4 * 2^-24 * |t64| — three roundings of exact binary32 inputs: the subtraction, the reciprocal, the product, each
    half an ulp (2^-24 relative).  The boxes' centres and extents are dyadic, so the corners c -/+ e are exact in binary32 too."""
    rng = np.random.default_rng(20260412)
    boxes = [(0, 0, 0, 1, 2, 3), (5.5, -2.25, 7.125, 0.5, 0.25, 4), (-130, 40, 9, 12, 1.5, 0.375), (2.0**-6, 2.0**-5, -(2.0**-6), 2.0**-3, 2.0**-2, 2.0**-4)]  # (the smallest hit distance is a tenth of an extent: above the 0.001 rule)
    assert all(float(np.float32(c + s * e)) == c + s * e for b in boxes for c, e in zip(b[:3], b[3:]) for s in (-1, 1))
    origins, directions, rows = random_face_rays(rng, boxes, 10000)
    camera = rt_amd.Scene.named("basic").describe(64, 36)
    for b, box in enumerate(boxes):
        mine = [i for i, r in enumerate(rows) if r[2] == b]
        pod = box_ref.scene_pod(camera, boxes=[(*box, 0)])
        t, kind, index, normal = box_ref.closest_hit(pod, origins[mine], directions[mine])
        for j, i in enumerate(mine):
            _, _, _, axis, sign, inside = rows[i]
            hit64, t64, axis64, sign64 = slab_test_float64(origins[i].astype(np.float64), directions[i].astype(np.float64), np.array(box[:3]), np.array(box[3:]))
            assert hit64 and (axis64, sign64) == (axis, sign), (i, "the float64 rule does not find the face the ray was aimed at")
            assert kind[j] == box_ref.KIND_BOX and index[j] == 0, i
            want_normal = [0.0, 0.0, 0.0]
            want_normal[axis] = float(sign)
            assert list(normal[j]) == want_normal, (i, inside)
            assert abs(float(t[j]) - t64) <= 4 * 2.0**-24 * abs(t64), (i, float(t[j]), t64)


def test_an_accepted_box_hits_distance_is_oracle_hits_box(kat_scene):
    origins, directions, _ = box_ref.known_answer_rays()
    rng = np.random.default_rng(3)
    more_o = rng.uniform(-12, 12, (2000, 3)).astype(np.float32)
    aims = np.where(rng.integers(2, size=(2000, 1)) == 0, rng.uniform(-1, 1, (2000, 3)) * (1, 2, 3), rng.uniform(-1, 1, (2000, 3)) + (10, 2, 0))  # points of boxes 0 / 1 and of box 2
    more_d = aims - more_o
    more_d = (more_d / np.linalg.norm(more_d, axis=1, keepdims=True)).astype(np.float32)
    origins, directions = np.concatenate([origins, more_o]), np.concatenate([directions, more_d])
    t, kind, index, _ = box_ref.closest_hit(kat_scene, origins, directions)
    seen = 0
    for i in np.flatnonzero(kind == box_ref.KIND_BOX):
        box = box_ref.KAT_BOXES[int(index[i])]
        hit, want = oracle.hits_box(origins[i], directions[i], box[:3], box[3:6])
        assert hit and np.float32(want).view(np.uint32) == t[i].view(np.uint32), i
        seen += 1
    assert seen > 200


def test_the_golden_box_frame_regenerates_identically():
    """tests/golden/boxes_64x36_spp20.npz (tools/gen_golden.py): boxes.toml through the restatement, both scatter tables."""
    golden = np.load(GOLDEN / "boxes_64x36_spp20.npz")
    scene = rt_amd.Scene.load(SCENES_DIR / "boxes.toml").set_sampling(int(golden["spp"]), int(golden["max_bounces"]))
    assert (scene.describe(64, 36).n_spheres, scene.describe(64, 36).n_planes, scene.describe(64, 36).n_boxes) == (2, 1, 3)
    for sm, suffix in ((False, ""), (True, "_sm")):
        rgba, rgb, stats = box_ref.render(scene.describe(64, 36), 64, 36, seed=int(golden["seed"]), sm_materials=sm)
        assert np.array_equal(rgba, golden["rgba" + suffix])
        assert np.array_equal(rgb.view(np.uint32), golden["rgb" + suffix].view(np.uint32))
        assert stats["segments"] == int(golden["segments" + suffix])
    # and the boxes are in it: the oracle's frame of the same scene, which never hits a box, differs
    flat, _, _ = oracle.render(scene.describe(64, 36), 64, 36, seed=int(golden["seed"]), want_rgb=False)
    assert (flat != golden["rgba"]).mean() > 0.05
