"""The serial restatement of adaptive sampling's update step (tests/native/adaptive_reference.cpp over rt_amd/csrc/adaptive_rules.hpp —
the text the kernel runs) against a float64 numpy restatement of DESIGN.md §3.11, on random states and on hand-made cases.

The state words must be EQUAL.  That asks for inputs on which the rule's one inequality is not a matter of rounding: binary32 forms
d = S2 - S1 * mean from two numbers of size S2 with a relative error of a few 2^-24 each, so se2 carries an absolute error of about
m / (m - 1) * 2^-22 * mean^2, while lim = (threshold * (mean + floor))^2 is 9e-4 * mean^2 at the defaults.  The random pixels are
therefore of two kinds — flat ones, whose passes differ by rounding only (se2 within that error of 0: far below lim), and noisy ones,
whose y swings by half its level from pass to pass (se2 above a hundredth of mean^2: far above) — and the test asserts, in float64, that every judged pixel's se2 is off
lim by more than a tenth of lim, which is orders of magnitude beyond the error.  The moments must be equal wherever float64 rounds to
the same float, and everywhere within the eight roundings a moment has behind it."""
import numpy as np
import pytest

from tests import adaptive_reference as ref

F32, F64 = np.float32, np.float64
STOPPED, COUNT = ref.STOPPED, ref.COUNT
NAN = np.float32(np.nan)


def step64(pass_sum, moments, state, pass_samples, first, whole, p):
    """§3.11 in float64 on float32 inputs: -> (S1, S2, n, converged, se2, lim), each [H, W]; a stopped pixel keeps its words."""
    s = pass_sum.astype(F64)
    stopped = np.zeros(state.shape, dtype=bool) if first else (state & STOPPED) != 0
    n_before = np.zeros(state.shape, dtype=np.int64) if first else (state & COUNT).astype(np.int64)
    n = np.where(stopped, n_before, n_before + pass_samples)
    with np.errstate(all="ignore"):
        y = ((s[..., 0] + s[..., 1]) + s[..., 2]) / (3 * pass_samples)
        S1 = y if first else moments[..., 0].astype(F64) + y
        S2 = y * y if first else moments[..., 1].astype(F64) + y * y
        m = n // pass_samples
        mean = S1 / m
        d = S2 - S1 * mean
        var = np.where(d > 0, d, 0.0) / (m - 1)
        se2 = var / m
        lim = (F64(p.threshold) * (mean + F64(p.floor))) ** 2
        converged = (n >= p.min_samples) & (m >= 2) & (se2 <= lim)  # (a NaN compares false)
    if not whole:
        converged = np.zeros(state.shape, dtype=bool)
        S1, S2 = (moments[..., 0].astype(F64), moments[..., 1].astype(F64)) if not first else (S1, S2)
    if not first:
        S1 = np.where(stopped, moments[..., 0].astype(F64), S1)
        S2 = np.where(stopped, moments[..., 1].astype(F64), S2)
    converged = converged | stopped
    return S1, S2, n, converged, se2, lim, stopped


def stop3x3(converged):
    """A pixel stops when it and its neighbours inside the frame are converged (outside counts as converged)."""
    padded = np.pad(converged, 1, constant_values=True)
    h, w = converged.shape
    out = np.ones((h, w), dtype=bool)
    for dy in range(3):
        for dx in range(3):
            out &= padded[dy : dy + h, dx : dx + w]
    return out


def state64(state, first, n, converged, stopped):
    after = n.astype(np.uint32) | np.where(stop3x3(converged), STOPPED, np.uint32(0))
    return after if first else np.where(stopped, state, after)


def check_step(accum, pass_sum, moments, state, pass_samples, first, whole, p, judged_margin=True):
    got_moments, got_state, rgba, rgb, active = ref.step(accum, pass_sum, moments, state, pass_samples, first, whole, p)
    S1, S2, n, converged, se2, lim, stopped = step64(pass_sum, moments, state, pass_samples, first, whole, p)
    judged = ~stopped & whole & (n >= p.min_samples) & (n // pass_samples >= 2) & np.isfinite(se2) & np.isfinite(lim)
    if judged_margin and judged.any():  # the inputs leave the inequality to no rounding (module docstring)
        assert (np.abs(se2 - lim)[judged] > 0.1 * lim[judged]).all()
    want_state = state64(state, first, n, converged, stopped)
    assert np.array_equal(got_state, want_state), f"{(got_state != want_state).sum()} state words differ"
    assert active == int(((want_state & STOPPED) == 0).sum())
    if whole:
        touched = ~stopped
        for k, want in enumerate((S1, S2)):
            got = got_moments[..., k]
            with np.errstate(all="ignore"):
                same_rounding = want.astype(F32).view(np.uint32) == got.view(np.uint32)
                close = np.abs(got.astype(F64) - want) <= 8 * 2.0**-24 * np.abs(want)
            nan_both = np.isnan(want) & np.isnan(got)
            assert (same_rounding | close | nan_both)[touched].all(), f"moment {k}"
    if not first:  # a stopped pixel's words are kept as they are
        assert np.array_equal(got_moments.view(np.uint32)[stopped], moments.view(np.uint32)[stopped])
        assert np.array_equal(got_state[stopped], state[stopped])
    if not whole:  # a short pass updates the state words only
        assert np.array_equal(got_moments.view(np.uint32), np.asarray(moments, dtype=F32).view(np.uint32))
    # every pixel is finished from the running sum and its OWN sample count
    count = (got_state & COUNT).astype(F32)
    with np.errstate(all="ignore"):
        assert np.array_equal(rgb.view(np.uint32), (np.asarray(accum, dtype=F32) / count[..., None]).view(np.uint32))
    assert ((rgba & 255) == 255).all()
    return got_moments, got_state


def random_passes(rng, height, width, passes, pass_samples):
    """Per pass a [H, W, 3] fold: flat pixels (the same value every pass, up to its last bits) and noisy ones (the pixel's level times
    1.5, 0.5, 1.5, ... give or take a tenth: never two passes that happen to agree)."""
    flat = rng.random((height, width)) < 0.6
    level = rng.uniform(0.2, 1.5, size=(height, width, 3))
    out = []
    for k in range(passes):
        noisy = level * (1.0 + 0.5 * (-1) ** k + rng.uniform(-0.1, 0.1, size=(height, width, 1)))
        value = np.where(flat[..., None], level * (1.0 + rng.uniform(-1e-7, 1e-7, size=(height, width, 3))), noisy)
        out.append((value * pass_samples).astype(F32))
    return out, flat


@pytest.mark.parametrize("height,width,pass_samples,passes", [(23, 37, 16, 6), (16, 16, 48, 4), (1, 1, 16, 3), (3, 50, 32, 5)])
def test_random_accumulations_against_float64(height, width, pass_samples, passes):
    rng = np.random.default_rng(100 * height + width)
    p = ref.params(min_samples=2 * pass_samples)
    sums, flat = random_passes(rng, height, width, passes, pass_samples)
    moments = np.full((height, width, 2), NAN, dtype=F32)
    state = np.full((height, width), 0xFFFFFFFF, dtype=np.uint32)  # (the first pass reads neither)
    accum = np.zeros((height, width, 3), dtype=F32)
    for k, pass_sum in enumerate(sums):
        active = np.ones((height, width), dtype=bool) if k == 0 else (state & STOPPED) == 0
        accum = np.where(active[..., None], pass_sum if k == 0 else accum + pass_sum, accum).astype(F32)
        stale = np.where(active[..., None], pass_sum, NAN)  # a stopped pixel was not traced: its pass sum must not be read
        moments, state = check_step(accum, stale, moments, state, pass_samples, k == 0, True, p)
    stopped = (state & STOPPED) != 0
    assert not stopped[~flat].any()  # a noisy pixel never stops at these sample counts ...
    if height * width > 1:
        assert stopped.any() and (state & COUNT)[stopped].min() == 2 * pass_samples  # ... flat neighbourhoods stop at min_samples
    # the short last pass: 8 more samples for whoever is active, nobody is judged
    check_step(accum, np.full_like(accum, NAN), moments, state, 8, False, False, p)


def frame(height, width, value):
    return np.full((height, width, 3), value, dtype=F32)


def test_a_pixel_with_one_pass_never_converges():
    """m = 1: var is 0 / 0; min_samples cannot be below two passes, so the verdict is `m >= 2`'s and the NaN's."""
    p = ref.params(threshold=1e30)
    moments, state = check_step(frame(2, 2, 16.0), frame(2, 2, 16.0), np.zeros((2, 2, 2)), np.zeros((2, 2)), 16, True, True, p)
    assert (state == 16).all() and np.array_equal(moments[..., 0], np.full((2, 2), 1.0, dtype=F32))


def test_min_samples_not_yet_reached():
    p = ref.params(threshold=1e30, min_samples=64)
    moments, state = np.zeros((2, 2, 2), dtype=F32), np.zeros((2, 2), dtype=np.uint32)
    accum = frame(2, 2, 0.0)
    for k in range(4):
        accum = accum + 16.0
        moments, state = check_step(accum, frame(2, 2, 16.0), moments, state, 16, k == 0, True, p)
        assert ((state & STOPPED) != 0).all() == (k == 3), k  # 16, 32, 48: not yet; 64: every pixel


def test_var_is_clamped_at_0():
    """Three identical passes of y = 0.1: S2 - S1 * mean comes out below zero in binary32 (3 roundings of y * y on one side, S1 * S1 / 3
    on the other), the clamp makes it 0, and a threshold of 0 still converges — 0 <= 0.  (Binary32's own business: no float64 here.)"""
    s = F32(1.6)  # r = g = b: y = fl(fl(3.2 + 1.6) / 48)
    p = ref.params(threshold=0.0, floor=0.0)
    moments, state = np.zeros((1, 1, 2), dtype=F32), np.zeros((1, 1), dtype=np.uint32)
    found_negative = False
    for k in range(6):
        moments, state, _, _, _ = ref.step(frame(1, 1, s * (k + 1)), frame(1, 1, s), moments, state, 16, k == 0, True, p)
        S1, S2 = moments[0, 0]
        m = F32(k + 1)
        d = F32(S2 - F32(S1 * F32(S1 / m)))
        if k >= 1 and d <= 0:
            found_negative = found_negative or d < 0
            assert (state[0, 0] & STOPPED) != 0, k  # clamped to 0, and 0 <= 0
            break
    assert (state[0, 0] & STOPPED) != 0
    # ... and with moments no accumulation leaves, d = 1 - 2 * 1 = -1 for certain: var = 0, not -1
    moments, state, _, _, _ = ref.step(frame(1, 1, 32.0), frame(1, 1, 16.0), np.array([[[1.0, 0.0]]], dtype=F32), np.array([[16]], dtype=np.uint32), 16, False, True, p)
    assert tuple(moments[0, 0]) == (2.0, 1.0) and state[0, 0] == (32 | STOPPED)


def test_a_nan_in_the_pass_sum_never_converges():
    p = ref.params(threshold=1e30)
    for channel in range(3):
        moments, state = np.zeros((3, 3, 2), dtype=F32), np.zeros((3, 3), dtype=np.uint32)
        accum = frame(3, 3, 0.0)
        for k in range(4):
            pass_sum = frame(3, 3, 16.0)
            if k == 0:
                pass_sum[1, 1, channel] = NAN
            accum = accum + pass_sum
            moments, state = check_step(accum, pass_sum, moments, state, 16, k == 0, True, p)
        assert ((state & STOPPED) == 0).all()  # the centre never converges, and keeps all eight neighbours going
        assert (state == 64).all()
    # ... and neither does an infinite threshold product: inf * 0
    assert ref.check(ref.params(threshold=float("inf")))[0] == 1


@pytest.mark.parametrize("noisy", [(0, 0), (0, 4), (3, 0), (3, 4), (0, 2), (3, 2), (1, 0), (2, 4), (1, 2)])
def test_the_3x3_rule_at_corners_edges_and_inside(noisy):
    """One pixel that does not converge in a 4 x 5 frame of flat ones: exactly its in-frame neighbourhood keeps going."""
    height, width = 4, 5
    p = ref.params()
    moments, state = np.zeros((height, width, 2), dtype=F32), np.zeros((height, width), dtype=np.uint32)
    accum = frame(height, width, 0.0)
    for k in range(2):
        pass_sum = frame(height, width, 16.0)
        pass_sum[noisy] = 0.0 if k == 0 else 32.0
        accum = accum + pass_sum
        moments, state = check_step(accum, pass_sum, moments, state, 16, k == 0, True, p)
    ys, xs = np.mgrid[0:height, 0:width]
    near = (np.abs(ys - noisy[0]) <= 1) & (np.abs(xs - noisy[1]) <= 1)
    assert np.array_equal((state & STOPPED) == 0, near) and (state & COUNT == 32).all()


def test_a_stopped_pixel_is_kept_as_it_is():
    """Its words survive a pass whose pass sum (stale scratch) is NaN, whatever its neighbours do; and stopping is monotone."""
    p = ref.params()
    state = np.full((3, 3), 32, dtype=np.uint32)
    state[1, 1] |= STOPPED
    moments = np.tile(np.array([2.0, 2.0], dtype=F32), (3, 3, 1))
    moments[1, 1] = (0.25, 7.0)  # (words no update would leave)
    pass_sum = np.random.default_rng(3).uniform(0, 64, size=(3, 3, 3)).astype(F32)  # noisy neighbours
    pass_sum[1, 1] = NAN
    accum = frame(3, 3, 40.0)
    new_moments, new_state = check_step(accum, pass_sum, moments, state, 16, False, True, p)
    assert new_state[1, 1] == (32 | STOPPED) and tuple(new_moments[1, 1]) == (0.25, 7.0)
    assert (np.delete(new_state.ravel(), 4) == 48).all()
    _, _, rgba, rgb, active = ref.step(accum, pass_sum, moments, state, 16, False, True, p)
    assert active == 8 and rgb[1, 1, 0] == F32(40.0) / F32(32.0) and rgb[0, 0, 0] == F32(40.0) / F32(48.0)


def test_the_parameter_check_and_the_refusals_of_a_step():
    assert ref.check(ref.params()) == (0, "")
    assert ref.pass_size(0) == 16 and ref.pass_size(33) == 48
    for bad in (dict(threshold=-1.0), dict(floor=float("nan")), dict(min_samples=31)):
        status, message = ref.check(ref.params(**bad))
        assert status == 1 and next(iter(bad)) in message
        with pytest.raises(ValueError):
            ref.step(frame(1, 1, 1.0), frame(1, 1, 1.0), np.zeros((1, 1, 2)), np.zeros((1, 1)), 16, True, True, ref.params(**bad))
    with pytest.raises(ValueError):  # a whole pass is whole chunks
        ref.step(frame(1, 1, 1.0), frame(1, 1, 1.0), np.zeros((1, 1, 2)), np.zeros((1, 1)), 24, True, True)
