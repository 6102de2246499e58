"""Tone mapping's rules on the CPU: the serial restatement (tests/native/tonemap_reference.cpp over
rt_amd/csrc/tonemap_rules.hpp, the kernels' own text) against a numpy float32 restatement written from DESIGN's text — equality is
exact: numpy's float32 + - x / sqrt are the same IEEE operations — and against float64: the meter against the geometric mean it
stands for, the curves against their formulas.  No GPU."""
import numpy as np
import pytest

from tests import tonemap_reference as ref

F32 = np.float32
U = 2.0 ** -24  # the unit roundoff of float32: one correctly rounded operation is off by at most this, relatively


# ---- DESIGN.md §3.15 in numpy float32 -------------------------------------------------------------------------------------------------
def luminance(rgb):
    rgb = np.asarray(rgb, dtype=F32)
    return (F32(0.2126) * rgb[..., 0] + F32(0.7152) * rgb[..., 1]) + F32(0.0722) * rgb[..., 2]


def by_hand(rgb, p, state=None):
    """(mapped float32[H, W, 3], rgba uint32[H, W], state uint32[8]) as §3.15 says, integers in python's, floats in numpy float32."""
    rgb = np.asarray(rgb, dtype=F32)
    state = np.zeros(8, dtype=np.uint32) if state is None else np.array(state, dtype=np.uint32)
    with np.errstate(all="ignore"):
        if p.exposure > 0:
            exposure = F32(p.exposure)
            state[:] = 0
            state[:2] = np.array([exposure], dtype=F32).view(np.uint32)[0]
        else:
            y = luminance(rgb).reshape(-1)
            is_counted = (y == y) & (y > 0) & (y < np.inf)
            bits = y[is_counted].view(np.uint32).astype(np.int64)
            bins = np.bincount(np.clip((bits >> 20) - 888, 0, 255), minlength=256)
            n = int(bins.sum())
            target, kept, q = F32(1.0), 0, 0
            if n:
                lo, hi = n * p.low_permille // 1000, n * p.high_permille // 1000
                kept, s, before = n - lo - hi, 0, 0
                for b in range(256):
                    after = before + int(bins[b])
                    s += b * max(0, min(after, n - hi) - max(before, lo))
                    before = after
                q = 256 * s // kept
                metered = np.array([(888 << 20) + (q << 12) + (1 << 19)], dtype=np.uint32).view(F32)[0]
                target = F32(p.key) / metered
                target = F32(p.min_exposure) if target < F32(p.min_exposure) else target
                target = F32(p.max_exposure) if target > F32(p.max_exposure) else target
            prev = state[:1].view(F32)[0]
            if p.adaptation < 1 and prev == prev and prev > 0 and prev < np.inf:
                exposure = prev + F32(p.adaptation) * (target - prev)
            else:
                exposure = target
            state[:] = [np.array([exposure], dtype=F32).view(np.uint32)[0], np.array([target], dtype=F32).view(np.uint32)[0], n, y.size - n, kept, q, 0, 0]
        v = rgb * F32(exposure)
        v = np.where(v > 0, v, F32(0))
        v = np.where(v < F32(2.0 ** 20), v, F32(2.0 ** 20))
        if p.curve == ref.REINHARD:
            scale = (F32(1) + luminance(v) / (F32(p.white) * F32(p.white))) / (F32(1) + luminance(v))
            o = v * scale[..., None]
        elif p.curve == ref.ACES:
            o = (v * (F32(2.51) * v + F32(0.03))) / (v * (F32(2.43) * v + F32(0.59)) + F32(0.14))
        else:
            o = v
        # pack_mean: square root, clamp to [0, 1], x 255.99999, truncate; r, g, b, 255 from the top byte down
        root = np.sqrt(o)
        clamped = np.where(root > 1, F32(1), np.where(root >= 0, root, F32(0)))
        byte = (clamped * F32(255.99999)).astype(np.uint32)
        rgba = (byte[..., 0] << 24) | (byte[..., 1] << 16) | (byte[..., 2] << 8) | np.uint32(255)
    assert o.dtype == F32
    return o, rgba.astype(np.uint32), state


def same(a, b):
    """bit for bit, NaNs included"""
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def assert_equal_to_by_hand(rgb, p, state=None):
    got, want = ref.frame(rgb, p, state), by_hand(rgb, p, state)
    assert np.array_equal(got[2], want[2]), (ref.info_of(got[2]), ref.info_of(want[2]))
    assert same(got[0], want[0])
    assert np.array_equal(got[1], want[1])
    return got


# ---- the restatement equals the text ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lights", "lights_sm", "basic"])
@pytest.mark.parametrize("curve", ref.CURVES)
def test_fixture_frames(name, curve):
    out, rgba, state = assert_equal_to_by_hand(ref.fixture_frames()[name], ref.params(curve=curve))
    info = ref.info_of(state)
    assert info["counted"] + info["skipped"] == 64 * 36 and info["skipped"] == 0 and 0 < info["kept"] <= info["counted"]
    assert np.isfinite(out).all()


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (3, 5), (1, 257), (36, 64), (41, 70)])
@pytest.mark.parametrize("curve", ref.CURVES)
def test_random_frames_over_forty_octaves(shape, curve):
    rgb = ref.noise(*shape, seed=shape[0] * 1000 + shape[1])
    assert_equal_to_by_hand(rgb, ref.params(curve=curve))
    assert_equal_to_by_hand(rgb, ref.params(curve=curve, low_permille=0, high_permille=0, key=1.0))
    assert_equal_to_by_hand(rgb, ref.params(curve=curve, low_permille=333, high_permille=666, white=0.5))


@pytest.mark.parametrize("name", list(ref.constructed_cases()))
def test_constructed_cases(name):
    rgb, p = ref.constructed_cases()[name]
    assert_equal_to_by_hand(rgb, p)


def test_the_fixture_is_why_this_exists():
    """The lights frame: float means up to 4, a fourteenth of its channels above 1 — flat white under the renderer's own finish."""
    rgb = ref.fixture_frames()["lights"]
    assert rgb.max() == 4.0 and 0.06 < (rgb > 1).mean() < 0.08


# ---- the hand-made cases, by what must come out ---------------------------------------------------------------------------------------
def test_every_pixel_in_one_bin():
    rgb, p = ref.constructed_cases()["one bin"]
    info = ref.info_of(ref.frame(rgb, p)[2])
    assert info["counted"] == 35 and info["skipped"] == 0 and info["kept"] == 35 - 1 - 0 and info["mean_q8"] == 100 * 256  # floor(35 x 50 / 1000) = 1, floor(35 x 20 / 1000) = 0
    assert info["target"] == float(F32(0.18) / F32(ref.bin_centre(100))) == info["exposure"]
    assert np.array_equal(np.flatnonzero(ref.histogram(rgb)), [100])


def test_every_pixel_skipped():
    rgb, p = ref.constructed_cases()["all skipped"]
    out, rgba, state = ref.frame(rgb, p)
    assert ref.info_of(state) == {"exposure": 1.0, "target": 1.0, "counted": 0, "skipped": 35, "kept": 0, "mean_q8": 0}
    assert ref.histogram(rgb)[256] == 35 and not ref.histogram(rgb)[:256].any()
    assert np.isfinite(out).all()  # NaN and negatives to 0, +inf to the cap


def test_both_end_bins():
    rgb, p = ref.constructed_cases()["end bins"]
    h = ref.histogram(rgb)
    assert h[0] == 9 + 9 and h[255] == 9 + 8 and h.sum() == 35  # 35 pixels cycling four values: 9, 9, 9, 8
    assert ref.info_of(ref.frame(rgb, p)[2])["mean_q8"] == 256 * 255 * 17 // 35


def test_a_rank_cut_inside_a_bin_and_on_a_bin_edge():
    rgb, p = ref.constructed_cases()["cut inside a bin"]
    assert np.array_equal(ref.histogram(rgb)[[60, 200]], [20, 15])
    info = ref.info_of(ref.frame(rgb, p)[2])  # floor(3.5) = 3 off each end: 17 of bin 60, 12 of bin 200
    assert info["kept"] == 29 and info["mean_q8"] == 256 * (60 * 17 + 200 * 12) // 29
    rgb, p = ref.constructed_cases()["cut on a bin edge"]
    assert np.array_equal(ref.histogram(rgb)[[40, 80, 120, 160]], [10, 10, 10, 10])
    info = ref.info_of(ref.frame(rgb, p)[2])
    assert info["kept"] == 20 and info["mean_q8"] == 256 * 100  # bins 80 and 120 whole, 40 and 160 not at all
    rgb, p = ref.constructed_cases()["no trim"]
    info = ref.info_of(ref.frame(rgb, p)[2])
    assert info["kept"] == info["counted"] == 35 and info["mean_q8"] == 256 * (60 * 20 + 200 * 15) // 35


def test_one_metered_pixel_survives_999_permille():
    rgb, p = ref.constructed_cases()["one metered pixel, 999 permille"]
    info = ref.info_of(ref.frame(rgb, p)[2])
    assert info["counted"] == 1 and info["skipped"] == 34 and info["kept"] == 1 and info["mean_q8"] == 77 * 256


def test_the_clamps_are_hit():
    for name, limit in (("min clamp", 0.5), ("max clamp", 2.0)):
        rgb, p = ref.constructed_cases()[name]
        info = ref.info_of(ref.frame(rgb, p)[2])
        assert info["target"] == limit == info["exposure"]


def test_adaptation():
    rgb = ref.fixture_frames()["lights"]
    target = ref.info_of(ref.frame(rgb, ref.params())[2])["target"]
    eased = ref.params(adaptation=0.25)
    for previous in (0.0, float("nan"), float("inf"), -2.0):  # no valid exposure before: the target at once
        state = np.zeros(8, dtype=np.uint32)
        state[:1] = np.array([previous], dtype=F32).view(np.uint32)
        assert ref.info_of(assert_equal_to_by_hand(rgb, eased, state)[2])["exposure"] == target
    state = np.zeros(8, dtype=np.uint32)
    state[:1] = np.array([2.0], dtype=F32).view(np.uint32)
    info = ref.info_of(assert_equal_to_by_hand(rgb, eased, state)[2])
    assert info["exposure"] == float(F32(2.0) + F32(0.25) * (F32(target) - F32(2.0))) and info["target"] == target
    assert ref.info_of(assert_equal_to_by_hand(rgb, ref.params(adaptation=1.0), state)[2])["exposure"] == target  # 1: the previous one is not read
    # three frames on one record: each eases from the one before
    record, frames = np.zeros(8, dtype=np.uint32), [ref.fixture_frames()[name] for name in ("lights", "basic", "lights_sm")]
    exposures = []
    for f in frames:
        record = assert_equal_to_by_hand(f, eased, record)[2]
        exposures.append(ref.info_of(record)["exposure"])
    assert exposures[0] == target and len(set(exposures)) == 3


def test_manual_exposure_meters_nothing():
    rgb, p = ref.constructed_cases()["manual exposure"]
    state = np.full(8, 0xDEADBEEF, dtype=np.uint32)
    out, _, state = ref.frame(rgb, p, state)
    assert ref.info_of(state) == {"exposure": float(F32(0.37)), "target": float(F32(0.37)), "counted": 0, "skipped": 0, "kept": 0, "mean_q8": 0} and not state[6:].any()
    assert same(out, by_hand(rgb, p)[0])


@pytest.mark.parametrize("curve", ref.CURVES)
def test_hostile_channels(curve):
    name = {ref.NONE: "none", ref.REINHARD: "reinhard", ref.ACES: "aces"}[curve]
    rgb, p = ref.constructed_cases()[f"hostile channels, {name}"]
    out, rgba, _ = ref.frame(rgb, p)
    assert np.isfinite(out).all() and (out >= 0).all()
    cap = F32(2.0 ** 20)
    if curve == ref.NONE:
        assert np.array_equal(out[0, :6], np.array([[0, 1, 2], [cap, 0.5, 0.25], [0, 4, 0], [cap, cap, cap], [0, 0, cap], [0, 0, 0]], dtype=F32))
    assert np.array_equal(out[0, 5], [0, 0, 0]) and rgba[0, 5] == 0x000000FF and rgba[0, 3] == 0xFFFFFFFF


# ---- against float64 ------------------------------------------------------------------------------------------------------------------
def test_the_meter_stays_within_its_derived_bound_of_the_geometric_mean():
    """low = high = 0 and every luminance in [2^-16, 2^16): log2 of the metered luminance against the mean of log2 Y in float64.
    The bound: a float's exponent + mantissa understates its log2 by at most log2(1 + m) - m <= 0.0861 (at
    m = 1 / ln 2 - 1), on the metered side and on the pixels' side, so up to 0.0861 either way; a bin's centre is within 1/16 octave
    of any value in it; the floor of q loses at most 1/256 bin = 1/2048 octave.  No looser."""
    bound = 0.0861 + 1 / 16 + 1 / 2048
    p = ref.params(low_permille=0, high_permille=0)
    worst = 0.0
    frames = [ref.fixture_frames()[name] for name in ("lights", "lights_sm", "basic")]
    frames += [ref.noise(41, 70, seed=s, low=-15.0, high=15.0) for s in range(4)]
    frames += [ref.grey(5, 7, [v]) for v in (2.0 ** -15.99, 1.0, 1.4426950408889634, 1.999, 2.0 ** 15.99, 3.0e-5)]
    for rgb in frames:
        y = luminance(rgb).astype(np.float64).reshape(-1)
        assert ((y >= 2.0 ** -16) & (y < 2.0 ** 16)).all()
        info = ref.info_of(ref.frame(rgb, p)[2])
        assert info["kept"] == y.size
        metered = np.array([(888 << 20) + (info["mean_q8"] << 12) + (1 << 19)], dtype=np.uint32).view(F32)[0]
        off = np.log2(np.float64(metered)) - np.log2(y).mean()
        print(f"meter: log2 L - mean log2 Y = {off:+.4f} octave (bound {bound:.4f})")
        worst = max(worst, abs(off))
        assert abs(off) <= bound
    rgb = ref.fixture_frames()["lights"]  # what the defaults make of the lights frame, against its untrimmed geometric mean
    print(f"lights fixture: metered {0.18 / ref.info_of(ref.frame(rgb, ref.params())[2])['target']:.4f}, geometric mean {np.exp2(np.log2(luminance(rgb).astype(np.float64)).mean()):.4f}")
    assert worst > 0.01  # (the check can see something)


def test_the_curves_against_their_float64_formulas():
    """Every operand is finite and not negative, so no rounding error is amplified by cancellation: a sum's relative error is at most
    the larger of its terms' plus one rounding, a product's or quotient's the sum of its operands' plus one.  With u = 2^-24:
      v = c e                                   1
      NONE                                      1
      ACES  numerator  v (2.51 v + 0.03):       3 of its own, and the error of v twice (degree 2)          5
            denominator v (2.43 v + 0.59) + 0.14:  4 of its own, the error of v twice                       6
            the quotient                        5 + 6 + 1 = 12
      REINHARD  Yv: three products, two sums in depth 3, the error of v once                               4
            Yv / white^2: white^2 is one product, the quotient one more                                   6
            1 + that: 7;  1 + Yv: 5;  their quotient: 13;  v times it: 13 + 1 + 1 = 15
    first order in u; one more u covers the higher orders (15 u^2 is far below u).  The float64 formulas use the float32 constants'
    own values (2.51f is not 2.51) and inputs that keep every intermediate a normal float."""
    rng = np.random.default_rng(11)
    c = np.exp2(rng.uniform(-20, 20, size=(64, 64, 3))).astype(F32)
    c[0, 0] = [2.0 ** 20, 2.0 ** 20, 2.0 ** 20]
    for exposure in (2.0 ** -10, 0.37, 1.0, 2.0 ** 10):
        e = np.float64(F32(exposure))
        v = np.minimum(c.astype(np.float64) * e, 2.0 ** 20)
        for curve, budget in ((ref.NONE, 1 + 1), (ref.ACES, 12 + 1), (ref.REINHARD, 15 + 1)):
            p = ref.params(curve=curve, exposure=exposure, white=3.0)
            got = ref.frame(c, p)[0].astype(np.float64)
            if curve == ref.ACES:
                k = [np.float64(F32(x)) for x in (2.51, 0.03, 2.43, 0.59, 0.14)]
                want = (v * (k[0] * v + k[1])) / (v * (k[2] * v + k[3]) + k[4])
            elif curve == ref.REINHARD:
                k = [np.float64(F32(x)) for x in (0.2126, 0.7152, 0.0722)]
                yv = k[0] * v[..., 0] + k[1] * v[..., 1] + k[2] * v[..., 2]
                want = v * ((1 + yv / np.float64(F32(3.0)) ** 2) / (1 + yv))[..., None]
            else:
                want = v
            off = np.abs(got / want - 1).max()
            print(f"curve {curve} at exposure {exposure:g}: worst relative error {off / U:.2f} u (bound {budget} u)")
            assert off <= budget * U
