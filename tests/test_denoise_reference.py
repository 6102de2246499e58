"""The guide-buffer denoiser on the CPU: its serial restatement over the kernels' own per-pixel text
(tests/native/denoise_reference.cpp + rt_amd/csrc/denoise_rules.hpp, g++ alone).  What the filter must preserve exactly, an independent
evaluation of the same formulas in numpy float64, the parameter check, `finish` against the oracle's pack, and — the point of it —
that the default-filtered 16-spp frame is nearer the 1024-spp frame than the unfiltered one.  tests/test_gpu_denoise.py then holds the
device to this restatement bit for bit."""
import functools

import numpy as np
import pytest

import rt_amd
from oracle import binding as oracle
from tests import denoise_reference as ref

F32 = np.float32
W, H = 37, 23


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def synthetic_guide(rng, height=H, width=W, sky=0.25):
    """A guide nobody traced: random unit normals, depths of 1 .. 10, albedos, five primitives, and blocks of sky."""
    normal = rng.normal(size=(height, width, 3))
    normal /= np.linalg.norm(normal, axis=-1, keepdims=True)
    guide = np.zeros((height, width, 8), dtype=F32)
    guide[..., 0:3] = normal
    guide[..., 3] = rng.uniform(1.0, 10.0, size=(height, width))
    guide[..., 4:7] = rng.uniform(0.0, 1.0, size=(height, width, 3))
    ids = rng.integers(1, 6, size=(height, width)).astype(np.uint32)
    is_sky = np.kron(rng.random((-(-height // 4), -(-width // 4))) < sky, np.ones((4, 4), dtype=bool))[:height, :width]
    guide[is_sky, 0:4] = (0.0, 0.0, 0.0, -1.0)
    ids[is_sky] = 0
    guide[..., 7] = ids.view(F32)
    return guide, is_sky


def smooth_guide(height=H, width=W):
    """One surface seen head on: every edge-stopping term of the guide is 1, the colour term alone steers."""
    guide = np.zeros((height, width, 8), dtype=F32)
    guide[..., 2] = 1.0
    guide[..., 3] = 5.0
    guide[..., 4:7] = 0.5
    guide[..., 7] = np.full((height, width), 1, dtype=np.uint32).view(F32)
    return guide


# ---- the parameters -------------------------------------------------------------------------------------------------------------
def test_defaults_pass_the_check_and_are_the_products():
    p = ref.params()
    assert ref.check(p) == (0, "")
    from rt_amd import renderer

    assert bytes(p) == bytes(renderer.denoise_default_params())  # (one denoise.cpp, compiled into both)


@pytest.mark.parametrize(
    "field,value",
    [("iterations", 7), ("normal_squarings", 9), ("sigma_colour", 0.0), ("sigma_colour", float("nan")), ("sigma_albedo", -1.0), ("sigma_albedo", float("inf")), ("sigma_depth", 0.0), ("sigma_depth", float("-inf"))],
)
def test_out_of_range_parameters_are_refused_with_the_fields_name(field, value):
    status, message = ref.check(ref.params(**{field: value}))
    assert status == 1 and field in message, (status, message)
    with pytest.raises(ValueError, match=field):
        ref.filter(np.zeros((2, 2, 3), dtype=F32), smooth_guide(2, 2), ref.params(**{field: value}))


def test_every_value_in_range_passes():
    for iterations in range(7):
        for squarings in range(9):
            assert ref.check(ref.params(iterations=iterations, normal_squarings=squarings))[0] == 0
    assert ref.check(ref.params(sigma_colour=1e-30, sigma_albedo=1e30, sigma_depth=1e-3))[0] == 0


def test_finish_is_the_path_tracers_finish():
    rng = np.random.default_rng(3)
    means = np.concatenate([rng.uniform(0.0, 1.5, size=(500, 3)), [[0.0, 1.0, 4.0], [-1.0, np.nan, np.inf], [0.25, 0.5, 1e-40]]]).astype(F32)
    got = ref.finish(means)
    for mean, packed in zip(means, got):
        with np.errstate(invalid="ignore"):
            root = np.sqrt(mean.astype(F32))  # correctly rounded in binary32
        assert packed == oracle.pack(float(root[0]), float(root[1]), float(root[2]))


# ---- what the filter preserves exactly ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [0.0, 0.5, 1.0])
def test_a_constant_image_comes_back_bit_identical_for_every_iteration_count_on_any_guide(value):
    rng = np.random.default_rng(11)
    image = np.full((H, W, 3), value, dtype=F32)
    for guide in (synthetic_guide(rng)[0], smooth_guide()):
        for iterations in range(7):
            out, rgba = ref.filter(image, guide, ref.params(iterations=iterations))
            assert np.array_equal(bits(out), bits(image)), (value, iterations)
            assert np.array_equal(rgba, ref.finish(image))


@pytest.mark.parametrize("squarings", range(1, 9))
def test_a_step_between_regions_with_perpendicular_normals_is_kept_bit_for_bit(squarings):
    guide = smooth_guide()
    guide[:, W // 2 :, 0:3] = (1.0, 0.0, 0.0)  # the right half faces +x, the left half +z: same depth, same albedo, same primitive
    image = np.full((H, W, 3), 0.25, dtype=F32)
    image[:, W // 2 :] = 1.0
    for iterations in (1, 3, 6):
        out, _ = ref.filter(image, guide, ref.params(iterations=iterations, normal_squarings=squarings, sigma_colour=100.0))  # (a colour term that would not stop anything)
        assert np.array_equal(bits(out), bits(image)), (squarings, iterations)


def test_sky_never_mixes_with_hit_pixels():
    rng = np.random.default_rng(12)
    guide, is_sky = synthetic_guide(rng)
    assert is_sky.any() and (~is_sky).any()
    image = rng.uniform(0.0, 1.0, size=(H, W, 3)).astype(F32)
    p = ref.params(iterations=4, sigma_colour=10.0)
    out, _ = ref.filter(image, guide, p)
    other_sky = image.copy()
    other_sky[is_sky] = rng.uniform(5.0, 9.0, size=(int(is_sky.sum()), 3))
    out_other_sky, _ = ref.filter(other_sky, guide, p)
    assert np.array_equal(bits(out[~is_sky]), bits(out_other_sky[~is_sky]))  # no hit pixel saw a sky pixel
    other_hits = image.copy()
    other_hits[~is_sky] = rng.uniform(5.0, 9.0, size=(int((~is_sky).sum()), 3))
    out_other_hits, _ = ref.filter(other_hits, guide, p)
    assert np.array_equal(bits(out[is_sky]), bits(out_other_hits[is_sky]))  # no sky pixel saw a hit pixel
    assert not np.array_equal(bits(out), bits(image))  # (and something was filtered)


@pytest.mark.parametrize("poison", [np.nan, np.inf, -np.inf])
def test_a_non_finite_pixel_neither_spreads_nor_changes(poison):
    rng = np.random.default_rng(13)
    image = rng.uniform(0.0, 1.0, size=(H, W, 3)).astype(F32)
    image[9, 17, 1] = poison
    for guide in (smooth_guide(), synthetic_guide(rng)[0]):
        for iterations in (1, 4, 6):
            out, _ = ref.filter(image, guide, ref.params(iterations=iterations, sigma_colour=5.0))
            assert np.array_equal(bits(out[9, 17]), bits(image[9, 17]))
            finite = np.isfinite(out).all(axis=-1)
            finite[9, 17] = True
            assert finite.all(), f"{(~finite).sum()} pixels caught the {poison}"
    # ... and its neighbours are what they would be if the pixel were not in the frame's sums at all: on a smooth guide with a colour term
    # that stops nothing, one iteration's weights are the spline's alone
    out, _ = ref.filter(image, smooth_guide(), ref.params(iterations=1, sigma_colour=1e18))
    h = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16])
    weights = np.outer(h, h)
    weights[2 + (9 - 10), 2 + (17 - 16)] = 0.0  # the tap of pixel (16, 10) that falls on the poisoned pixel
    window = image[8:13, 14:19].astype(np.float64)
    window[1, 3] = 0.0
    want = (weights[..., None] * window).sum(axis=(0, 1)) / weights.sum()
    assert np.allclose(out[10, 16], want, rtol=1e-5)


# ---- an independent evaluation: the same formulas in numpy float64 ----------------------------------------------------------------
def float64_filter(image, guide, p):
    """DESIGN.md §3.8's formulas, straight: for every pixel the 25 taps' weights and the weighted mean, in binary64, iteration after iteration."""
    height, width = image.shape[:2]
    colour = image.astype(np.float64)
    normal, depth, albedo = guide[..., 0:3].astype(np.float64), guide[..., 3].astype(np.float64), guide[..., 4:7].astype(np.float64)
    sky = guide[..., 7].copy().view(np.uint32) == 0
    spline = {0: 3 / 8, 1: 1 / 4, 2: 1 / 16}
    ys, xs = np.mgrid[0:height, 0:width]
    for i in range(p.iterations):
        step, sigma_colour = 2**i, float(p.sigma_colour) * 2.0**-i
        numerator, denominator = np.zeros_like(colour), np.zeros((height, width))
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                qy, qx = ys + dy * step, xs + dx * step
                inside = (qy >= 0) & (qy < height) & (qx >= 0) & (qx < width)
                qy, qx = np.clip(qy, 0, height - 1), np.clip(qx, 0, width - 1)
                w = np.full((height, width), spline[abs(dx)] * spline[abs(dy)])
                if dx or dy:
                    hits = ~sky & ~sky[qy, qx]
                    w_normal = np.maximum(0.0, (normal * normal[qy, qx]).sum(axis=-1)) ** (2 ** int(p.normal_squarings))
                    with np.errstate(divide="ignore", invalid="ignore"):
                        w_depth = 1.0 / (1.0 + ((depth - depth[qy, qx]) / (float(p.sigma_depth) * np.maximum(depth, depth[qy, qx]))) ** 2)
                    w_albedo = 1.0 / (1.0 + ((albedo - albedo[qy, qx]) ** 2).sum(axis=-1) / float(p.sigma_albedo) ** 2)
                    w_colour = 1.0 / (1.0 + ((colour - colour[qy, qx]) ** 2).sum(axis=-1) / sigma_colour**2)
                    w = w * np.where(hits, w_normal * w_depth * w_albedo, 1.0) * w_colour
                    w = np.where(sky != sky[qy, qx], 0.0, w)
                w = np.where(inside, w, 0.0)
                numerator += w[..., None] * colour[qy, qx]
                denominator += w
        colour = numerator / denominator[..., None]
    return colour


# The restatement rounds every operation to binary32 (unit roundoff u = 2^-24): about 30 roundings on a weight's way, 25 adds and a
# division per sum — some 60 u per iteration before the colour term feeds a pixel's error back into the next iteration's weights with a
# gain of up to c / sigma_colour_i, which no simple bound covers.  So: the largest deviation OBSERVED over the cases below is 4.6e-7
# relative (2 iterations, 50 taps; about 8 u); the tolerance is 4 x that.  It must stay below 1e-4 whatever is observed.
FLOAT64_TOLERANCE = 4 * 4.6e-7
assert FLOAT64_TOLERANCE < 1e-4


@pytest.mark.parametrize("iterations,squarings", [(1, 0), (2, 3), (3, 5)])
def test_the_restatement_is_the_formulas_evaluated_independently_in_float64(iterations, squarings):
    rng = np.random.default_rng(14)
    guide, _ = synthetic_guide(rng)
    guide[..., 0:3] = np.where(rng.random((H, W, 1)) < 0.7, F32((0.6, 0.0, 0.8)), guide[..., 0:3])  # (most normals agree, or hardly anything would be averaged)
    guide[..., 3] = np.where(guide[..., 3] > 0, F32(4.0) + rng.uniform(0.0, 0.3, size=(H, W)).astype(F32), guide[..., 3])
    image = rng.uniform(0.25, 1.0, size=(H, W, 3)).astype(F32)
    p = ref.params(iterations=iterations, normal_squarings=squarings, sigma_colour=2.0, sigma_albedo=1.0, sigma_depth=0.1)
    got, _ = ref.filter(image, guide, p)
    want = float64_filter(image, guide, p)
    deviation = float(np.max(np.abs(got.astype(np.float64) - want) / np.abs(want)))
    print(f"float64 check, {iterations} iterations, {squarings} squarings: largest relative deviation {deviation:.3e}")
    assert float(np.abs(got - image).max()) > 0.05  # (the case averages something)
    assert deviation <= FLOAT64_TOLERANCE, deviation


# ---- it denoises ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def frames(name, width=96, height=54):
    scene = rt_amd.Scene.named(name)
    noisy = oracle.render(scene.set_sampling(16).describe(width, height), width, height, seed=7)[1]
    truth = oracle.render(scene.set_sampling(1024).describe(width, height), width, height, seed=8)[1]
    guide = ref.compose_guide(scene.describe(width, height), width, height)
    return noisy, truth.astype(np.float64), guide


@pytest.mark.parametrize("name", ["basic", "dielectric"])
def test_the_default_filter_brings_a_16_spp_frame_nearer_the_1024_spp_frame(name):
    noisy, truth, guide = frames(name)
    filtered, _ = ref.filter(noisy, guide, None)
    before = float(np.mean((noisy.astype(np.float64) - truth) ** 2))
    after = float(np.mean((filtered.astype(np.float64) - truth) ** 2))
    print(f"{name} 96x54: mean squared error against 1024 spp, 16 spp unfiltered {before:.3e}, default-filtered {after:.3e}")
    assert after < before, "the defaults are wrong"
