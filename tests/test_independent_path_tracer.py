"""A SECOND restatement of the path, independent of oracle/cpu_ref.cpp: numpy, binary64, vectorised over all samples of a frame,
written from the reference's text — worker lambda and trace (src/renderers/mg_ray_tracer.cpp:155-201), test_planes / test_spheres
/ select (:36-102), lambert_scatter / metal_scatter (:110-140), screen_to_world (src/camera.hpp:42-48) — and from the stream
contract (the numpy generator of tests/test_oracle_kat.py, itself independent of the oracle's C++).

The oracle is unpinned (the reference has no tests and cannot be built here): the only tie between it and the reference is
one reading of the source.  This file is a second coding of that reading in another language, another precision and another
program structure (no recursion, no per-pixel loop, no float32 rounding anywhere), fed the SAME random numbers.  The two must
agree on every pixel to within what float32 rounding and the odd sample that falls on the other side of a silhouette can do."""
import numpy as np
import pytest

import rt_amd
from oracle import binding as oracle
from tests.fast_reference import render_f64  # (the restatement itself: shared with the per-pixel rule of RT_HIP_FLAG_FAST's builds)


CASES = [
    ("basic", None, 96, 54, 24, 10),
    ("dielectric", None, 96, 54, 16, 10),  # mg semantics: every kind but metal shades as lambert, albedo x reflectivity > 1 included
    ("basic_plane", None, 80, 45, 16, 6),
    ("dielectric_plane", ((0.2, 1.2, 7.0), (0.0, -0.15, -1.0)), 80, 45, 16, 10),  # a camera that is not axis-aligned
]


@pytest.mark.parametrize("name,camera,width,height,spp,bounces,sm_materials", [c + (False,) for c in CASES] + [("dielectric", None, 96, 54, 16, 10, True), ("dielectric_plane", None, 80, 45, 12, 10, True)])
def test_the_oracle_agrees_with_an_independent_float64_restatement(name, camera, width, height, spp, bounces, sm_materials):
    """(the last two cases: sm_ray_tracer's scatter table, where dielectrics refract — the path of hip_sm_ray_tracer)"""
    scene = rt_amd.Scene.named(name).set_sampling(spp, bounces)
    if camera:
        scene.set_camera(*camera)
    pod = scene.describe(width, height)
    seed = 12345
    _, oracle_mean, stats = oracle.render(pod, width, height, seed=seed, sm_materials=sm_materials)
    mine = render_f64(pod, width, height, seed, sm_materials)
    difference = np.abs(oracle_mean.astype(np.float64) - mine).max(axis=-1)
    # A sample that lands on the other side of a silhouette, of the min_hit_dist threshold or of the metal's absorption test
    # under float32 rounding changes a pixel's mean by up to (its weight)/spp — and everything downstream of it; such pixels
    # are rare.  Everywhere else the two agree to float32 rounding accumulated over a path.
    scale = max(1.0, float(mine.max()))
    assert np.median(difference) <= 1e-6 * scale, (name, np.median(difference))  # (measured: 3e-8 .. 4e-8)
    assert stats["primary_samples"] == width * height * spp
    if sm_materials:
        # A path that has been refracted INTO a sphere starts on its surface, and whether `e.e < r^2` calls that inside (far root:
        # the ray leaves through the far side) or outside (near root ~ 0 < min_hit_dist: the ray passes through the sphere as if it
        # were not there) is decided by the last bit of the hit position — in the reference as much as here.  float64 and float32
        # toss that coin differently, so pixels that see a refracting sphere agree only on average: the rest of the frame must
        # agree as closely as under mg semantics, the frame's mean colour to 1.5 % (measured: 0.4-0.5 %).
        assert (difference <= 2e-4 * scale).mean() >= 0.90, (name, (difference <= 2e-4 * scale).mean())
        assert np.allclose(oracle_mean.mean(axis=(0, 1)), mine.mean(axis=(0, 1)), rtol=1.5e-2), (oracle_mean.mean(axis=(0, 1)), mine.mean(axis=(0, 1)))
        return
    assert (difference <= 2e-4 * scale).mean() >= 0.995, (name, (difference <= 2e-4 * scale).mean(), np.sort(difference.ravel())[-10:])
    assert (difference <= 1e-5 * scale).mean() >= 0.98, (name, (difference <= 1e-5 * scale).mean())
    # the frame as a whole: the mean colour, to 5e-5 relative (measured: 1e-6 .. 7e-6) — a systematic difference (a wrong factor,
    # a wrong draw order, a wrong tie rule, a wrong column layout) shows here at once
    assert np.allclose(oracle_mean.mean(axis=(0, 1)), mine.mean(axis=(0, 1)), rtol=5e-5), (oracle_mean.mean(axis=(0, 1)), mine.mean(axis=(0, 1)))
