"""Guided upsampling's rules on the CPU: the geometry against exact rationals, and the pixel rule — bilinear values,
the sky / hit edge, orphans, non-finite taps, the min_weight switch — through the serial restatement (tests/native/upsample_reference.cpp
over rt_amd/csrc/upsample_rules.hpp, the kernel's own text).  No GPU."""
from fractions import Fraction

import numpy as np
import pytest

from tests import upsample_reference as ref

F32 = np.float32
SIZES = [(1, 1), (2, 1), (7, 3), (8, 4), (9, 3), (33, 33), (37, 1), (1921, 961)]


def exact_source(x, W, w):
    """u = ((2x + 1) w - W) / 2W as a rational: floor, and the two weights before rounding."""
    u = Fraction((2 * x + 1) * w - W, 2 * W)
    first = u.numerator // u.denominator
    frac = u - first
    return first, 1 - frac, frac


def nearest_f32(q: Fraction) -> np.float32:
    """A quotient of two integers below 2^24, correctly rounded to float32 (double's quotient is within half an ulp of double: no double rounding
    can matter unless the exact quotient lies within 2^-53 relative of a float32 tie, which a denominator below 2^24 cannot produce)."""
    return F32(np.float64(q.numerator) / np.float64(q.denominator))


@pytest.mark.parametrize("W,w", SIZES)
def test_source_of_equals_the_exact_rational_for_every_pixel(W, w):
    for x in range(W):
        first, b0, b1 = ref.source_of(x, W, w)
        want_first, want_b0, want_b1 = exact_source(x, W, w)
        assert first == want_first, (x, W, w)
        assert b0 == nearest_f32(want_b0) and b1 == nearest_f32(want_b1), (x, W, w)
        assert -1 <= first <= w - 1


@pytest.mark.parametrize("W,w", SIZES)
def test_exactly_the_expected_tap_is_outside_at_the_edges(W, w):
    left, _, _ = ref.source_of(0, W, w)
    right, _, right_b1 = ref.source_of(W - 1, W, w)
    if w < W:
        assert left == -1  # X0 outside, X1 = 0 inside
        assert right == w - 1  # X0 inside, X1 = w outside
    else:  # w == W: pixel x sits on low pixel x, the right neighbour has weight 0
        assert left == 0
        assert right == w - 1 and right_b1 == 0.0
    for x in range(W):  # never both outside
        first, _, _ = ref.source_of(x, W, w)
        assert 0 <= first or first + 1 <= w - 1
        assert first <= w - 1


def bilinear_by_hand(low, W, H):
    """The plain bilinear values in numpy float32, in the contract's order: the Y0 row first, X0 before X1; out = (sum of b c) / (sum of b)."""
    h, w = low.shape[:2]
    out = np.zeros((H, W, 3), dtype=F32)
    for y in range(H):
        fy, by0, by1 = ref.source_of(y, H, h)
        for x in range(W):
            fx, bx0, bx1 = ref.source_of(x, W, w)
            sw, s = F32(0), np.zeros(3, dtype=F32)
            for j, by in ((0, by0), (1, by1)):
                for i, bx in ((0, bx0), (1, bx1)):
                    qx, qy = fx + i, fy + j
                    if 0 <= qx < w and 0 <= qy < h:
                        b = F32(bx * by)
                        sw = F32(sw + b)
                        s = (s + (b * low[qy, qx]).astype(F32)).astype(F32)
            out[y, x] = (s / sw).astype(F32)
    return out


def test_a_4x4_from_2x2_over_one_surface_is_the_bilinear_frame():
    low = np.array([[[0.0, 0.25, 1.0], [1.0, 0.5, 0.0]], [[0.5, 0.75, 0.25], [0.125, 1.0, 0.5]]], dtype=F32)
    out, rgba, orphans = ref.frame(low, ref.hit_guide(2, 2), ref.hit_guide(4, 4))
    want = bilinear_by_hand(low, 4, 4)
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32))
    assert orphans == 0
    # worked by hand: the corners are their low pixel, pixel (1, 1) is 9/16, 3/16, 3/16, 1/16 of the four
    assert np.array_equal(out[0, 0], low[0, 0]) and np.array_equal(out[3, 3], low[1, 1])
    assert out[1, 1, 0] == F32(F32(0.5625) * low[0, 0, 0] + F32(0.1875) * low[0, 1, 0] + F32(0.1875) * low[1, 0, 0] + F32(0.0625) * low[1, 1, 0])
    assert np.array_equal(rgba, ref_finish(out))


def ref_finish(rgb):
    from tests import denoise_reference

    return denoise_reference.finish(rgb)


def test_a_sky_hit_edge_stays_an_edge():
    """Low frame 2 x 2: the left column sky with colour 0, the right column a hit with colour 1.  Every full pixel is exactly one of the
    two, by its own guide, wherever the edge of the full guide runs."""
    low = np.zeros((2, 2, 3), dtype=F32)
    low[:, 1] = 1.0
    guide_low = ref.hit_guide(2, 2)
    guide_low[:, 0] = ref.sky_guide(1, 1)[0, 0]
    guide_full = ref.hit_guide(8, 8)
    sky = np.zeros((8, 8), dtype=bool)
    for y in range(8):
        sky[y, : 3 + (y % 3)] = True  # a ragged edge between columns 2 and 5: pixels of both kinds have taps of both kinds
    sky[:, 0:2] = True
    sky[:, 6:8] = False
    guide_full[sky] = ref.sky_guide(1, 1)[0, 0]
    out, _, orphans = ref.frame(low, guide_low, guide_full)
    assert np.all(out[sky] == 0.0) and np.all(out[~sky] == 1.0)
    assert set(np.unique(out)) == {F32(0.0), F32(1.0)}
    # the outermost columns see only their own side's low column... except that a hit pixel in columns 6, 7 has no sky tap at all and
    # a sky pixel in columns 0, 1 no hit tap: nobody is an orphan here
    assert orphans == 0


def test_a_hit_pixel_among_sky_taps_is_an_orphan_and_takes_the_bilinear_mean():
    rng = np.random.default_rng(5)
    low = rng.random((2, 2, 3)).astype(F32)
    guide_full = ref.sky_guide(4, 4)
    guide_full[1, 2] = ref.hit_guide(1, 1)[0, 0]
    out, _, orphans = ref.frame(low, ref.sky_guide(2, 2), guide_full)
    want = bilinear_by_hand(low, 4, 4)
    assert orphans == 1
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32))  # (sky against sky is the bilinear weight alone: the whole frame is bilinear)
    # and with colours that tell the two rules apart: the orphan is the plain mean of all four, not of a subset
    assert np.array_equal(out[1, 2], want[1, 2])


def test_a_nan_tap_is_left_out_and_an_all_nan_neighbourhood_is_black():
    low = np.full((2, 2, 3), 0.25, dtype=F32)
    low[0, 0] = (np.nan, 0.5, 0.5)
    low[1, 1, 2] = np.inf
    out, rgba, orphans = ref.frame(low, ref.hit_guide(2, 2), ref.hit_guide(4, 4))
    assert np.all(np.isfinite(out))
    assert np.all(out[1:3, 1:3] == F32(0.25))  # the two finite taps' mean, renormalised
    assert np.array_equal(out[0, 3], low[0, 1]) and np.array_equal(out[3, 0], low[1, 0])
    # pixel (0, 0) has one tap inside the frame and it is not finite: no weight at all -> orphan, and no finite tap -> (0, 0, 0)
    assert np.all(out[0, 0] == 0.0) and np.all(out[3, 3] == 0.0)
    assert orphans == 2
    assert rgba[0, 0] == ref_finish(np.zeros((1, 3), dtype=F32))[0]
    everything = np.full((2, 2, 3), np.nan, dtype=F32)
    out, _, orphans = ref.frame(everything, ref.hit_guide(2, 2), ref.hit_guide(4, 4))
    assert np.all(out == 0.0) and orphans == 16


def test_min_weight_just_above_and_below_the_sum_switches_the_branch():
    """One low pixel, one full pixel: the only tap has bilinear weight 1, normal and depth terms 1 and an albedo term
    wa = 1 / (1 + d^2 / sigma^2) that the test computes in float32 as the rule does; sw = wa.  The guided branch and the orphan branch
    give the same colour here (one tap), so the orphan count tells them apart."""
    sigma = F32(0.1)
    d = F32(0.25)
    low = np.full((1, 1, 3), 0.5, dtype=F32)
    guide_low = ref.hit_guide(1, 1, albedo=(0.5, 0.5, 0.5))
    guide_full = ref.hit_guide(1, 1, albedo=(F32(0.5) + d, 0.5, 0.5))
    dd = F32(guide_full[0, 0, 4] - guide_low[0, 0, 4])
    sw = F32(F32(1.0) / F32(F32(1.0) + F32(F32(dd * dd) / F32(sigma * sigma))))
    assert 0.0 < sw < 1.0
    below, above = np.nextafter(sw, F32(0.0)), np.nextafter(sw, F32(1.0))
    for min_weight, want_orphans in ((below, 0), (sw, 0), (above, 1)):
        out, _, orphans = ref.frame(low, guide_low, guide_full, ref.params(sigma_albedo=float(sigma), min_weight=float(min_weight)))
        assert orphans == want_orphans, (min_weight, sw)
        assert np.all(out == F32(0.5))


def test_every_parameter_and_size_refusal_names_its_field():
    assert ref.check(ref.params())[0] == 0
    for fields, word in (({"normal_squarings": 9}, "normal_squarings"), ({"sigma_albedo": 0.0}, "sigma_albedo"), ({"sigma_albedo": float("nan")}, "sigma_albedo"), ({"sigma_depth": -1.0}, "sigma_depth"),
                         ({"sigma_depth": float("inf")}, "sigma_depth"), ({"min_weight": 0.0}, "min_weight"), ({"min_weight": 1.5}, "min_weight"), ({"min_weight": float("nan")}, "min_weight")):
        status, message = ref.check(ref.params(**fields))
        assert status == 1 and word in message, (fields, message)
    assert ref.check(ref.params(min_weight=1.0))[0] == 0
    assert ref.check_sizes(4, 4, 4, 4)[0] == 0 and ref.check_sizes(1 << 22, 1, 1, 1)[0] == 0
    for sizes, word in (((0, 4, 1, 1), "full frame"), (((1 << 22) + 1, 4, 1, 1), "full frame"), ((4, 4, 5, 1), "low frame"), ((4, 4, 1, 0), "low frame"), ((4, 4, 4, 5), "low frame")):
        status, message = ref.check_sizes(*sizes)
        assert status == 1 and word in message, (sizes, message)
