"""The rules of temporal accumulation on the CPU restatement (tests/native/reproject_reference.cpp: the serial loop
over rt_amd/csrc/reproject_rules.hpp, the text the kernel runs): what a pixel without history, a constant history, sky, a poisoned
history and a poisoned frame come out as; that the position check alone rejects what lies behind the previous camera; the geometry
against an independent binary64 projection; and that blending eight 16-spp frames brings the last one nearer the 1024-spp frame, at
rest and on a dolly.  No GPU."""
import functools

import numpy as np
import pytest

from oracle import binding as oracle
from tests import reproject_reference as ref
from tests import temporal_cases as cases
from tests.temporal_cases import bits

F32 = np.float32
W, H = 48, 27


def identical(a, b):
    return np.array_equal(bits(a), bits(b))


# ---- the rules ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["basic:rest", "planes_and_sky:rest", "orthographic:rest"])
def test_without_history_the_frame_passes_through_and_every_length_is_samples_in(name):
    pods, guides, _ = cases.case(name, W, H)
    rng = np.random.default_rng(1)
    image = rng.uniform(0.0, 2.0, size=(H, W, 3)).astype(F32)
    out, record, found = ref.frame(pods[0], guides[0], image, 24)
    assert identical(out, image) and found == 0
    ids = ref.ids_of(guides[0])
    assert np.array_equal(ref.ids_of(record), ids)
    assert np.all(record[..., 3] == 24.0)  # sky and hits alike: what the colour stands for
    assert identical(record[..., 4:7], guides[0][..., 0:3])
    assert np.all(record[ids == 0][:, 0:3] == 0.0)
    # the position is the centre ray's point at the guide's distance: an independent look at a hit pixel
    y, x = np.argwhere(ids != 0)[len(np.argwhere(ids != 0)) // 2]
    origin, direction = oracle.primary_ray(pods[0], W, H, int(x), int(y))
    assert np.allclose(record[y, x, 0:3], origin.astype(np.float64) + direction.astype(np.float64) * float(guides[0][y, x, 3]), rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("value", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("cap", [16, 64])
def test_a_constant_history_under_the_same_camera_stays_the_constant_and_the_lengths_add_up_to_the_cap(value, cap):
    """History and frame are the same constant: every blend is the constant bit for bit.  With 16 samples a frame and a cap that is a
    power of two every length on the way is a power-of-two multiple of the weights, so the bilinear mean of equal lengths is exact:
    after k frames the length is min(16 k, cap + 16)."""
    pods, guides, _ = cases.case("basic:rest", W, H)
    image = np.full((H, W, 3), value, dtype=F32)
    p = ref.params(max_history_samples=cap)
    frames = [(pods[0], guides[0], image, 16)] * 8
    hit = ref.ids_of(guides[0]) != 0
    assert hit.any() and not hit.all()
    for k, (out, record, found) in enumerate(ref.sequence(frames, p), start=1):
        assert identical(out, image), k
        lengths = record[..., 3]
        assert np.all(lengths[hit] == min(16 * k, cap + 16)), (k, np.unique(lengths[hit]))
        assert np.all(lengths[~hit] == 16)
        assert found == (hit.sum() if k > 1 else 0)


def test_sky_passes_through_and_keeps_no_history():
    pods, guides, _ = cases.case("planes_and_sky:rest", W, H)
    sky = ref.ids_of(guides[0]) == 0
    assert sky.any() and (~sky).any()
    rng = np.random.default_rng(2)
    first, second = (rng.uniform(0.0, 1.0, size=(H, W, 3)).astype(F32) for _ in range(2))
    steps = ref.sequence([(pods[0], guides[0], first, 16), (pods[1], guides[1], second, 32)])
    out, record, found = steps[1]
    assert identical(out[sky], second[sky])
    assert np.all(record[sky][:, 3] == 32.0) and np.all(record[sky][:, [0, 1, 2, 4, 5, 6]] == 0.0) and np.all(ref.ids_of(record)[sky] == 0)
    assert found == (~sky).sum()  # every hit pixel found itself
    assert not identical(out[~sky], second[~sky])


@pytest.mark.parametrize("poison", [np.nan, np.inf, -np.inf])
def test_a_non_finite_history_pixel_is_skipped_as_a_tap_and_never_spreads(poison):
    pods, guides, _ = cases.case("basic:rest", W, H)
    rng = np.random.default_rng(3)
    history = rng.uniform(0.0, 1.0, size=(H, W, 3)).astype(F32)
    _, record, _ = ref.frame(pods[0], guides[0], history, 16)
    history[20, 20, 1] = poison
    current = rng.uniform(0.0, 1.0, size=(H, W, 3)).astype(F32)
    out, new_record, found = ref.frame(pods[1], guides[1], current, 16, ref.matrix_of(pods[0]), history, record)
    assert np.isfinite(out).all() and np.isfinite(new_record[..., 0:7]).all()
    clean = history.copy()
    clean[20, 20] = 0.5
    out_clean, _, found_clean = ref.frame(pods[1], guides[1], current, 16, ref.matrix_of(pods[0]), clean, record)
    differing = (bits(out) != bits(out_clean)).any(axis=-1)
    assert differing[20, 20] and differing.sum() <= 4  # only the pixels one of whose four taps it was
    assert found in (found_clean, found_clean - 1)


@pytest.mark.parametrize("poison", [np.nan, np.inf])
def test_a_non_finite_current_pixel_passes_through_with_length_0(poison):
    pods, guides, _ = cases.case("basic:rest", W, H)
    matrix, history, record = cases.first_history("basic:rest", W, H)
    current = np.full((H, W, 3), 0.25, dtype=F32)
    hit = ref.ids_of(guides[1]) != 0
    assert hit[20, 7] and not hit[2, 7]
    current[20, 7, 2] = poison  # a hit pixel
    current[2, 7, 0] = poison  # and a sky pixel
    out, new_record, found = ref.frame(pods[1], guides[1], current, 16, matrix, history, record)
    for y in (20, 2):
        assert identical(out[y, 7], current[y, 7]) and new_record[y, 7, 3] == 0.0
    assert found == hit.sum() - 1
    # ... and as history it is nobody's tap
    again, _, found = ref.frame(pods[1], guides[1], np.full((H, W, 3), 0.25, dtype=F32), 16, matrix, out, new_record)
    assert np.isfinite(again).all() and found >= hit.sum() - 4


@pytest.mark.parametrize("name,form", [("surround:about_face", "pinhole"), ("surround_tilted:about_face", "eye"), ("orthographic:about_face", "general")])
def test_after_half_a_turn_no_pixel_finds_history_without_any_test_on_the_sign_of_w(name, form):
    pods, guides, _ = cases.case(name, W, H)
    for pod in pods:
        assert oracle.primary_ray(pod, W, H, 0, 0, want_form=True)[2] == form
    assert (ref.ids_of(guides[0]) > 1).any() and (ref.ids_of(guides[1]) > 1).any()  # spheres in sight on either side
    image = cases.ramp(W, H)
    _, record, _ = ref.frame(pods[0], guides[0], image, 16)
    loose = ref.params(position_tolerance=0.05, normal_threshold=-1.0)
    out, new_record, found = ref.frame(pods[1], guides[1], image, 16, ref.matrix_of(pods[0]), image, record, loose)
    assert found == 0 and identical(out, image)
    hit = ref.ids_of(guides[1]) != 0
    assert np.all(new_record[hit][:, 3] == 16.0)


def test_background_uncovered_behind_the_front_sphere_takes_no_history_from_the_sphere():
    """basic.toml, the camera stepping sideways: pixels that showed the matte sphere (id 2) now show the ground behind it (id 1)."""
    pods, guides, _ = cases.case("basic:dolly", W, H)
    before, after = ref.ids_of(guides[0]), ref.ids_of(guides[1])
    uncovered = (before == 2) & (after == 1)
    assert uncovered.sum() >= 3
    history = np.zeros((H, W, 3), dtype=F32)
    history[before == 2] = (100.0, 100.0, 100.0)  # the sphere glows in the history, everything else is black
    _, record, _ = ref.frame(pods[0], guides[0], history, 16)
    out, _, _ = ref.frame(pods[1], guides[1], np.zeros((H, W, 3), dtype=F32), 16, ref.matrix_of(pods[0]), history, record, ref.params(position_tolerance=1.0, normal_threshold=-1.0))
    assert np.all(out[after != 2] == 0.0)  # even with the position and normal checks wide open: the ids differ
    assert (out[after == 2] > 0.0).any()


# ---- geometry against an independent statement ------------------------------------------------------------------------------------
# The history colour is a ramp (r = x, g = y): what a pixel fetches is the bilinear mean of its taps' coordinates, that is (u, v) itself.
# The other side is numpy in binary64 from the same hit points: the previous matrix inverted by numpy, the projection, and the
# position check with its margin.  The largest deviation observed was 2.13e-5 pixels (dolly) and 1.69e-5 (yaw) — float rounding of u and
# v at coordinates up to 96 — and the bound is 4 x the larger.
GEOMETRY_TOLERANCE = 8.6e-5
GW, GH = 96, 54


@pytest.mark.parametrize("move", ["dolly", "yaw"])
def test_the_fetched_coordinates_are_a_binary64_projection_of_the_same_hit_points(move):
    pods, guides, _ = cases.case(f"basic_plane:{move}", GW, GH)
    image = cases.ramp(GW, GH)
    _, record, _ = ref.frame(pods[0], guides[0], image, 16)
    p = ref.params(max_history_samples=1 << 20, position_tolerance=0.05, normal_threshold=0.9)
    out, new_record, found = ref.frame(pods[1], guides[1], np.zeros_like(image), 1, ref.matrix_of(pods[0]), image, record, p)
    had = new_record[..., 3] > 1.0
    assert had.sum() == found
    fetched = out.astype(np.float64) * 17.0 / 16.0  # out = (h x 16 + 0 x 1) / 17

    # the independent side
    forward64 = np.linalg.inv(ref.matrix_of(pods[0]).astype(np.float64).reshape(4, 4))
    points = new_record[..., 0:3].astype(np.float64)
    clip = np.concatenate([points, np.ones((GH, GW, 1))], axis=-1) @ forward64.T
    u = (clip[..., 0] / clip[..., 3] + 1.0) * 0.5 * GW - 0.5
    v = (1.0 - clip[..., 1] / clip[..., 3]) * 0.5 * GH - 0.5
    inside = (u > -1.0) & (u < GW) & (v > -1.0) & (v < GH)
    near_edge = (np.abs(u + 1.0) < 1e-3) | (np.abs(u - GW) < 1e-3) | (np.abs(v + 1.0) < 1e-3) | (np.abs(v - GH) < 1e-3)
    x0, y0 = np.floor(u).astype(int), np.floor(v).astype(int)
    ids, prev_ids = ref.ids_of(guides[1]), ref.ids_of(record)
    depth = guides[1][..., 3].astype(np.float64)
    reach = float(F32(0.05)) * depth
    want = np.zeros((GH, GW), dtype=bool)
    on_the_margin = np.zeros((GH, GW), dtype=bool)
    wu, wv, ww = np.zeros((GH, GW)), np.zeros((GH, GW)), np.zeros((GH, GW))
    for y, x in np.argwhere(inside & (ids != 0)):
        for j in (0, 1):
            for i in (0, 1):
                qx, qy = x0[y, x] + i, y0[y, x] + j
                if not (0 <= qx < GW and 0 <= qy < GH) or prev_ids[qy, qx] != ids[y, x]:
                    continue
                if float(np.dot(record[qy, qx, 4:7].astype(np.float64), guides[1][y, x, 0:3].astype(np.float64))) < 0.9:
                    continue
                distance = float(np.linalg.norm(record[qy, qx, 0:3].astype(np.float64) - points[y, x]))
                if abs(distance - reach[y, x]) <= 1e-3 * reach[y, x]:
                    on_the_margin[y, x] = True
                if distance > reach[y, x]:
                    continue
                w = ((u[y, x] - x0[y, x]) if i else (1.0 - (u[y, x] - x0[y, x]))) * ((v[y, x] - y0[y, x]) if j else (1.0 - (v[y, x] - y0[y, x])))
                ww[y, x] += w
                wu[y, x] += w * qx
                wv[y, x] += w * qy
        want[y, x] = ww[y, x] > 0.0
    left_out = on_the_margin | near_edge
    assert left_out.sum() <= 0.05 * GW * GH, left_out.sum()
    assert np.array_equal(had[~left_out], want[~left_out]), f"{(had != want)[~left_out].sum()} pixels disagree about having history"
    both = had & want & ~left_out
    assert both.sum() > 0.8 * (ids != 0).sum()  # (the move keeps most of what is no sky)
    deviation = max(float(np.abs(fetched[..., 0][both] - wu[both] / ww[both]).max()), float(np.abs(fetched[..., 1][both] - wv[both] / ww[both]).max()))
    print(f"{move}: {both.sum()} pixels compared, {left_out.sum()} left out, largest deviation {deviation:.3e} pixels")
    assert deviation <= GEOMETRY_TOLERANCE, deviation


# ---- it helps -----------------------------------------------------------------------------------------------------------------------
HW, HH, FRAMES = 96, 54, 8
CAMERAS = {"basic": (0.0, 1.0, 3.0), "dielectric": (0.0, 1.0, 7.0)}
DOLLY = {"basic": 0.07, "dielectric": 0.14}  # world units along +x per frame (tools/temporal_tune.py)


@functools.lru_cache(maxsize=None)
def eight_frames(name, moving):
    frames = []
    for step in range(FRAMES):
        x, y, z = CAMERAS[name]
        pod = cases.toml_scene(name, HW, HH, (x + (DOLLY[name] * step if moving else 0.0), y, z), cases.FORWARD, spp=16)
        frames.append((pod, cases.guide_of(pod, HW, HH), oracle.render(pod, HW, HH, seed=1 + step)[1], 16))
    x, y, z = CAMERAS[name]
    last = cases.toml_scene(name, HW, HH, (x + (DOLLY[name] * (FRAMES - 1) if moving else 0.0), y, z), cases.FORWARD, spp=1024)
    return frames, oracle.render(last, HW, HH, seed=100)[1].astype(np.float64)


@pytest.mark.parametrize("moving", [False, True], ids=["rest", "dolly"])
@pytest.mark.parametrize("name", ["basic", "dielectric"])
def test_eight_blended_16_spp_frames_are_nearer_the_1024_spp_frame_than_the_last_one_alone(name, moving):
    frames, truth = eight_frames(name, moving)
    if moving:  # the whole move crosses at least a tenth of the frame's width: where frame 0 saw the last frame's sphere points
        first, last = frames[0], frames[-1]
        image = cases.ramp(HW, HH)
        start = ref.frame(first[0], first[1], image, 16)
        moved = ref.frame(last[0], last[1], np.zeros_like(image), 1, ref.matrix_of(first[0]), start[0], start[1], ref.params(max_history_samples=1 << 20))
        had = (moved[1][..., 3] > 1.0) & (ref.ids_of(last[1]) > 1)
        shift = np.abs(moved[0][..., 0][had].astype(np.float64) * 17.0 / 16.0 - np.broadcast_to(np.arange(HW)[None, :], (HH, HW))[had])
        assert had.sum() > 20 and float(np.median(shift)) >= HW / 10, float(np.median(shift))
    steps = ref.sequence(frames)  # the default parameters
    assert steps[-1][2] > 0.8 * (ref.ids_of(frames[-1][1]) != 0).sum()  # (most of what is no sky found history)
    alone = float(np.mean((frames[-1][2].astype(np.float64) - truth) ** 2))
    blended = float(np.mean((steps[-1][0].astype(np.float64) - truth) ** 2))
    print(f"{name} {'dolly' if moving else 'rest'} 96x54: mean squared error against 1024 spp, last 16-spp frame {alone:.3e}, blended {blended:.3e}")
    assert blended < alone, "the defaults are wrong"
