"""The CPU restatement of RT_HIP_FLAG_THIN_LENS (tests/native/lens_reference.cpp) on its own, without a GPU: with a radius
of 0 it IS the oracle; its draws, disk and ray agree with an independent binary64 numpy statement written from the contract's text and
fed the same step words; every lens ray of a pixel passes the pinhole ray's focus-plane point; a sample draws exactly one step more
than the oracle's; and a sphere off the focus plane is blurred.

Measured (`python -m tests.test_lens_reference` prints them): over the three cameras, 8 pixels and 24 samples each the restatement's ray
deviates from the numpy statement by at most 2.37e-7 per component (an origin component: half an ulp of a coordinate near 5; the
directions' worst is 8.9e-8).  BOUND below is 4 x that, 9.5e-7.  A lens ray passes its pinhole ray's focus-plane point at a distance of
at most 1.13e-7 x focus; the bound is BOUND x focus for every camera.  The three cameras are rt's axis-aligned one, a tilted one, and
for the guarded eye form the tilted camera's matrix with every entry times 2^-52 (the same view: tests/lens_reference.py,
guarded_squarely).  The parity tests' guarded matrix is not used HERE: it bends w until its corner rays graze the focus plane (cosine
0.019), where any ray's crossing point is ill-conditioned; the GPU tests hold the device to the restatement through it, bit for bit."""
import numpy as np
import pytest

import rt_amd
from oracle import binding as oracle
from tests import lens_reference as lens_ref

LENS = (0.08, 3.2)
BOUND = 9.5e-7


def cameras(width, height, spp=24):
    axis = lens_ref.named_scene("basic", lens_ref.AXIS_CAMERA, spp=spp).describe(width, height)
    tilted = lens_ref.named_scene("basic", lens_ref.TILTED_CAMERA, spp=spp).describe(width, height)
    scaled = lens_ref.guarded_squarely(lens_ref.named_scene("basic", lens_ref.TILTED_CAMERA, spp=spp).describe(width, height))
    for pod, form in ((axis, "pinhole"), (tilted, "eye"), (scaled, "guarded")):
        assert lens_ref.words(pod, width, height, LENS)[3] == lens_ref.FORM_OF[form]
    return {"pinhole": axis, "eye": tilted, "guarded": scaled}


@pytest.mark.parametrize("name", ["basic", "dielectric"])
@pytest.mark.parametrize("sm", [False, True])
def test_without_an_aperture_it_is_the_oracle(name, sm):
    pod = rt_amd.Scene.named(name).set_sampling(20).describe(64, 36)
    want_rgba, want_rgb, want = oracle.render(pod, 64, 36, seed=3, sm_materials=sm)
    for lens in (None, (0.0, 4.0)):
        rgba, rgb, stats = lens_ref.render(pod, 64, 36, lens, seed=3, sm_materials=sm)
        assert np.array_equal(rgba, want_rgba) and np.array_equal(rgb.view(np.uint32), want_rgb.view(np.uint32)) and stats["segments"] == want["segments"]
    blurred, _, _ = lens_ref.render(pod, 64, 36, (0.1, 2.0), seed=3, sm_materials=sm)
    assert (blurred != want_rgba).mean() > 0.2


# ---- the independent statement: binary64, from the text of the contract --------------------------------------------------------
def numpy_disk(ka, kb):
    x, y = ka * 2.0**-23 - 1.0, kb * 2.0**-23 - 1.0
    if abs(x) > abs(y):
        major, minor, first = x, y, True
    else:
        major, minor, first = y, x, False
    if major == 0.0:
        return 0.0, 0.0
    psi = (minor / major) * (np.pi / 4)
    return (major * np.cos(psi), major * np.sin(psi)) if first else (major * np.sin(psi), major * np.cos(psi))


def numpy_ray(pinhole, eye, words, ka, kb):
    """draws -> disk -> ray: L = U lx + V ly, t = focus / (d . fwd), origin = E + L, direction = normalised d t - L"""
    o, d = pinhole[:3].astype(np.float64), pinhole[3:].astype(np.float64)
    u, v, fwd, focus = words[0:3].astype(np.float64), words[3:6].astype(np.float64), words[6:9].astype(np.float64), float(words[9])
    lx, ly = numpy_disk(float(ka), float(kb))
    lens_point = u * lx + v * ly
    cosine = float(d @ fwd)
    if not cosine > 0.0 or not np.isfinite(focus / cosine):
        return o, d
    toward = d * (focus / cosine) - lens_point
    return eye.astype(np.float64) + lens_point, toward / np.linalg.norm(toward)


def deviations(width=48, height=27):
    worst_origin = worst_direction = 0.0
    worst_focus = {}  # per camera: the largest distance at which a lens ray passes its pinhole ray's focus-plane point, over focus
    for form, pod in cameras(width, height).items():
        status, words, eye, _ = lens_ref.words(pod, width, height, LENS)
        assert status == 0
        for x, y in [(0, 0), (width - 1, 0), (0, height - 1), (width - 1, height - 1), (width // 2, height // 2), (7, 19), (33, 5), (21, 13)]:
            for sample in range(24):
                got, pinhole, k, _ = lens_ref.ray(pod, width, height, LENS, x, y, sample, seed=5)
                want_o, want_d = numpy_ray(pinhole, eye, words, k[2], k[3])
                worst_origin = max(worst_origin, float(np.abs(got[:3] - want_o).max()))
                worst_direction = max(worst_direction, float(np.abs(got[3:] - want_d).max()))
                # the point where the pinhole's ray crosses the focus plane (fwd . (P - E) = focus), and how far the lens ray passes from it, in binary64
                fwd = words[6:9].astype(np.float64)
                cosine = float(pinhole[3:].astype(np.float64) @ fwd)
                if cosine > 0:
                    target = eye.astype(np.float64) + pinhole[3:].astype(np.float64) * (LENS[1] / cosine)
                    from_origin, along = target - got[:3].astype(np.float64), got[3:].astype(np.float64)
                    passes_at = np.linalg.norm(np.cross(from_origin, along)) / np.linalg.norm(along)
                    worst_focus[form] = max(worst_focus.get(form, 0.0), float(passes_at) / LENS[1])
    return worst_origin, worst_direction, worst_focus


def test_the_ray_is_the_numpy_statements_and_passes_the_focus_point():
    worst_origin, worst_direction, worst_focus = deviations()
    print(f"origin {worst_origin:.3g} direction {worst_direction:.3g} focus-plane miss over its scale {worst_focus}")
    assert worst_origin <= BOUND and worst_direction <= BOUND
    assert set(worst_focus) == {"pinhole", "eye", "guarded"}
    for form, miss in worst_focus.items():
        assert miss <= BOUND, form


def test_a_sample_draws_exactly_one_step_more():
    """sample 0: the lens step alone (no jitter) where the oracle's draws nothing; every later sample: jitter, then lens"""
    pod = cameras(48, 27)["pinhole"]
    for sample in (0, 1, 2, 15, 16, 23):
        _, _, plain_k, plain_steps = lens_ref.ray(pod, 48, 27, None, 11, 7, sample, seed=9)
        _, _, k, steps = lens_ref.ray(pod, 48, 27, LENS, 11, 7, sample, seed=9)
        assert plain_steps == (1 if sample else 0) and steps == plain_steps + 1
        assert tuple(k[:2]) == tuple(plain_k[:2])  # the jitter is the oracle's
        if sample == 0:
            assert tuple(k[:2]) == (1 << 23, 1 << 23)


def test_the_pinhole_ray_is_the_oracles():
    pod = cameras(48, 27)["eye"]
    _, pinhole, k, _ = lens_ref.ray(pod, 48, 27, LENS, 5, 6, 3, seed=2)
    origin, direction = oracle.primary_ray(pod, 48, 27, 5, 6, float(k[0]), float(k[1]))[:2]
    assert np.array_equal(np.asarray(origin, dtype=np.float32), pinhole[:3]) and np.array_equal(np.asarray(direction, dtype=np.float32), pinhole[3:])


def test_a_sphere_off_the_focus_plane_is_blurred():
    """One grey lambert sphere against the sky, max_bounces 1 (every hit is black, every miss sky): a pixel is 'partial' when its 64
    samples disagree.  On the focus plane the lens changes next to nothing about the silhouette; far in front of it the silhouette is a
    wide ring of partial pixels."""
    camera = lens_ref.named_scene("basic", lens_ref.AXIS_CAMERA).describe(64, 36)  # eye (0, 1, 3), looking down -z

    def partial_pixels(distance, focus):
        radius = 0.25 * distance / 3.0  # (the same size on screen at every distance)
        pod = lens_ref.scene_pod(camera, spheres=[(0.0, 1.0, 3.0 - distance, radius, 0)], spp=64, bounces=1)
        _, rgb, _ = lens_ref.render(pod, 64, 36, (0.15, focus), seed=4)
        _, sky, _ = lens_ref.render(lens_ref.scene_pod(camera, spheres=[(0.0, -50.0, 60.0, 0.1, 0)], spp=64, bounces=1), 64, 36, (0.15, focus), seed=4)  # (the sphere behind the camera)
        hit_share = 1.0 - rgb.sum(axis=2) / sky.sum(axis=2)
        return int(((hit_share > 0.05) & (hit_share < 0.95)).sum())

    on_plane, off_plane = partial_pixels(3.0, 3.0), partial_pixels(1.0, 6.0)
    assert off_plane > 2 * on_plane and off_plane > 40, (on_plane, off_plane)


if __name__ == "__main__":
    print("origin %.3g direction %.3g focus-plane miss over its scale %s" % deviations())
