"""The CPU restatement of RT_HIP_FLAG_EMISSION (tests/native/light_reference.cpp) on its own, without a GPU: it is the
oracle where no material is a light, it gives known answers where the answer can be known (the furnace, one-bounce frames), and a
binary64 path tracer written from §3.12's text agrees with it on a scene whose paths are deterministic."""
import numpy as np
import pytest

import rt_amd
from oracle import binding as oracle
from tests import light_reference as light_ref
from tests.conftest import GOLDEN


@pytest.mark.parametrize("name", ["basic", "dielectric"])
@pytest.mark.parametrize("sm", [False, True])
def test_without_a_light_it_is_the_oracle(name, sm):
    """1. An all-zero table (and -0.0f, which counts as zero): frame, float mean and counters of oracle.render, bit for bit."""
    pod = rt_amd.Scene.named(name).set_sampling(20).describe(64, 36)
    want_rgba, want_rgb, want = oracle.render(pod, 64, 36, seed=5, sm_materials=sm)
    for table in (None, np.full((pod.n_materials, 3), -0.0, dtype=np.float32)):
        rgba, rgb, stats = light_ref.render(pod, 64, 36, table, seed=5, sm_materials=sm)
        assert np.array_equal(rgba, want_rgba) and np.array_equal(rgb.view(np.uint32), want_rgb.view(np.uint32))
        assert stats["segments"] == want["segments"] and stats["primary_samples"] == want["primary_samples"]


@pytest.mark.parametrize("spp", [1, 16, 17, 20, 33])
def test_the_furnace(spp):
    """2. The camera at the centre of one sphere whose material is a light E = (0.25, 0.5, 2.0): every sample is exactly E, sums of
    equal powers of two are exact, so every pixel's float mean is exactly E; one segment per sample; blue clamps to 255."""
    width, height = 32, 18
    pod, table = light_ref.furnace(width, height, spp)
    for sm in (False, True):
        rgba, rgb, stats = light_ref.render(pod, width, height, table, seed=3, sm_materials=sm)
        assert np.array_equal(rgb.view(np.uint32), np.broadcast_to(np.array(light_ref.FURNACE_E, dtype=np.float32).view(np.uint32), rgb.shape))
        assert stats["segments"] == width * height * spp
        want = oracle.pack(*(float(np.sqrt(np.float32(v))) for v in light_ref.FURNACE_E))
        assert want & 0xFF00 == 0xFF00 and (rgba == want).all()


def sample0_rays(pod, width, height):
    rays = [oracle.primary_ray(pod, width, height, x, y) for y in range(height) for x in range(width)]
    return np.array([r[0] for r in rays]), np.array([r[1] for r in rays])


def test_one_bounce_frames_are_e_sky_or_zero():
    """3. max_bounces = 1 on lights.toml at spp 1 (sample 0 goes through the pixel centre): the sample is E where the primary ray's
    closest hit is the lamp, the sky where it misses, 0 where it hits anything else (the scattered ray has no bounce left)."""
    width, height = 64, 36
    pod = light_ref.lights_scene(spp=1, bounces=1).describe(width, height)
    origins, directions = sample0_rays(pod, width, height)
    _, kind, index, _ = oracle.closest_hit(pod, origins, directions)
    lamp = (kind == 1) & (index == 0)  # sphere 0 is the lamp
    want = np.zeros((width * height, 3), dtype=np.float32)
    want[lamp] = light_ref.LIGHTS_TABLE[1]
    for i in np.flatnonzero(kind == 0):
        want[i] = oracle.sky(float(directions[i][1]))
    assert lamp.sum() > 20 and (kind == 0).sum() > 100 and ((kind != 0) & ~lamp).sum() > 100
    for sm in (False, True):
        _, rgb, stats = light_ref.render(pod, width, height, light_ref.LIGHTS_TABLE, seed=8, sm_materials=sm)
        assert np.array_equal(rgb.reshape(-1, 3).view(np.uint32), want.view(np.uint32))
        assert stats["segments"] == width * height


def test_a_binary64_path_tracer_written_from_the_contract_agrees():
    """4. A roughness-0 metal sphere of albedo a (reflectivity 1), a lamp sphere and the sky, spp 1: sample 0 goes through the pixel centre and
    a mirror's scatter does not depend on its draws, so every path is deterministic — a^k . E, a^k . sky, or 0 (no bounce left).  Written
    from DESIGN.md §3.12 in float64: bounce check, closest hit (nothing nearer than 0.001), light -> throughput * emission and stop,
    miss -> throughput * sky.  Agreement to 1e-5 relative; a pixel whose float64 path has a hit / miss margin below 1e-4 is left out,
    and the float64 classification alone must keep that within 2 % of the frame."""
    width, height, bounces = 64, 36, 6
    albedo, emission = np.array([0.9, 0.6, 0.4]), np.array([3.0, 2.0, 0.5])
    camera = rt_amd.Scene.named("basic").describe(width, height)  # the eye at (0, 1, 3), looking down -z
    spheres = [(0.0, 1.0, 0.0, 1.0, 0), (2.2, 2.5, 0.5, 0.8, 1)]
    pod = light_ref.scene_pod(camera, spheres=spheres, spp=1, bounces=bounces, materials=[(light_ref.METAL, tuple(albedo), 0.0, 1.0), (light_ref.LAMBERT, (0.5, 0.5, 0.5), 0.0, 1.0)])
    table = np.array([(0, 0, 0), tuple(emission)], dtype=np.float32)
    _, rgb, _ = light_ref.render(pod, width, height, table, seed=2)

    origins, directions = sample0_rays(pod, width, height)
    o = origins.astype(np.float64)
    d = directions.astype(np.float64)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    n = len(o)
    throughput = np.ones((n, 3))
    value = np.zeros((n, 3))
    alive = np.ones(n, dtype=bool)
    risky = np.zeros(n, dtype=bool)
    last = np.full(n, -1)  # the sphere a ray starts on (a convex sphere cannot meet its own reflected ray)
    for _ in range(bounces):
        best_t = np.full(n, np.inf)
        best = np.full(n, -1)
        for k, (cx, cy, cz, r, _m) in enumerate(spheres):
            e = np.array([cx, cy, cz]) - o
            a = (e * d).sum(1)
            e2 = (e * e).sum(1)
            perp = np.sqrt(np.maximum(e2 - a * a, 0.0))
            disc = r * r - (e2 - a * a)
            f = np.sqrt(np.maximum(disc, 0.0))
            t = np.where(e2 < r * r, a + f, a - f)
            considered = alive & (last != k)
            risky |= considered & ((np.abs(perp - r) < 1e-4) | ((disc >= 0) & (np.abs(t - 1e-3) < 1e-4)))
            hit = considered & (disc >= 0) & (t >= 1e-3) & (t < best_t)
            best_t = np.where(hit, t, best_t)
            best = np.where(hit, k, best)
        miss = alive & (best < 0)
        sky_t = 0.5 * (d[:, 1] + 1.0)
        sky = np.stack([1.0 + (c - 1.0) * sky_t for c in (0.5, 0.7, 1.0)], axis=1)
        value[miss] = (throughput * sky)[miss]
        lamp = alive & (best == 1)
        value[lamp] = throughput[lamp] * emission
        mirror = alive & (best == 0)
        p = o + d * np.where(mirror, best_t, 0.0)[:, None]
        normal = (p - np.array(spheres[0][:3])) / spheres[0][3]
        reflected = d - 2.0 * (d * normal).sum(1)[:, None] * normal
        o = np.where(mirror[:, None], p, o)
        d = np.where(mirror[:, None], reflected / np.linalg.norm(reflected, axis=1, keepdims=True), d)
        throughput = np.where(mirror[:, None], throughput * albedo, throughput)
        last = np.where(mirror, 0, last)
        alive = mirror  # (a path still alive after the last bounce is worth 0: value stays 0)
    assert risky.mean() <= 0.02, risky.mean()
    got = rgb.reshape(-1, 3).astype(np.float64)[~risky]
    want = value[~risky]
    assert np.allclose(got, want, rtol=1e-5, atol=0.0)
    # every kind of path is in the frame: the lamp seen directly, the lamp in the mirror, the sky in the mirror, the sky
    direct = np.isclose(want, emission).all(1)
    mirrored = np.isclose(want, albedo * emission).all(1)
    assert direct.sum() > 20 and mirrored.sum() > 3 and (~direct & ~mirrored).sum() > 1000
