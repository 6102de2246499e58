"""Bloom's rules on the CPU: exact properties of the serial restatement over rt_amd/csrc/bloom_rules.hpp
(tests/bloom_reference.py) — what the device is then held to bit for bit (tests/test_gpu_bloom.py) — the level plan as a table, every
parameter refusal by its field's name, the parser's acceptances and refusals."""
import numpy as np
import pytest

import rt_amd
from rt_amd import capi
from tests import bloom_float64 as f64
from tests import bloom_reference as ref

F32 = np.float32
INVALID_ARGUMENT = 1
U = 2.0 ** -24  # half an ulp of 1: the relative error of one float32 rounding


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


# ---- nothing glows, nothing changes ---------------------------------------------------------------------------------------------------
def test_a_frame_below_the_knee_gets_a_zero_layer_and_keeps_its_bits():
    """Every channel below threshold - knee = 0.5: rq, soft and m - threshold are all <= 0, w = +0, every bright channel c x +0 = +0, and
    sums, products and quotients of +0 stay +0.  The inputs are not negative: out = in + gain x +0 keeps the bits of every in >= +0 (a
    -0 would come out as +0: -0 + +0 = +0)."""
    rgb = np.random.default_rng(1).uniform(0.0, 0.4999, size=(21, 37, 3)).astype(F32)
    rgb[0, 0] = 0.0
    out, layer, down, up = ref.frame(rgb, ref.params(), want_levels=True)
    assert not bits(layer).any() and all(not bits(l).any() for l in down + up)  # (bit pattern 0: +0 everywhere)
    assert np.array_equal(bits(out), bits(rgb))


def test_intensity_0_keeps_the_frame_s_bits():
    """gain = 0 / norm = +0: out = in + 0 x layer = in for every in >= +0.  (The layer is tent(up[0]) BEFORE the gain: not zero.)"""
    rgb = ref.noise(21, 37, seed=2)
    out, layer = ref.frame(rgb, ref.params(intensity=0.0))
    assert np.array_equal(bits(out), bits(rgb)) and layer.max() > 0


# ---- flat frames: the closed form, to the bit -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,height", [(1, 1), (5, 3), (37, 21)])
def test_flat_frames_are_the_closed_form(width, height):
    """Colour (2, 3, 4), threshold 1, knee 0: m = 4, w = 3, scale = 0.75, bright = (1.5, 2.25, 3) — few mantissa bits, so every tap sum
    is exact: the box gives 4 b / 4, a binomial pass 16 b, two of them 256 b / 256, the tent 0.75 v + 0.25 v = v.  Every level is flat
    at b on the way down, at b x (1 + 0.5 + ... ) on the way up, and the layer is b x norm."""
    p = ref.params(**ref.FLAT_PARAMS)
    rgb = ref.flat(height, width)
    plan = ref.plan(width, height, p)
    bright = np.array([1.5, 2.25, 3.0], dtype=F32)
    out, layer, down, up = ref.frame(rgb, p, want_levels=True)
    n = plan["levels"]
    assert plan["norm"] == F32(sum(0.5 ** i for i in range(n)))
    for i in range(n):
        assert np.array_equal(bits(down[i]), bits(np.broadcast_to(bright, down[i].shape))), i
        partial = F32(sum(0.5 ** k for k in range(n - i)))
        assert np.array_equal(bits(up[i]), bits(np.broadcast_to(bright * partial, up[i].shape))), i
    assert np.array_equal(bits(layer), bits(np.broadcast_to(bright * plan["norm"], layer.shape)))
    assert np.array_equal(bits(out), bits(rgb + plan["gain"] * layer))


# ---- impulses: the clamped indices --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in ref.constructed_cases() if n.startswith("impulse")])
def test_an_impulse_s_levels_sum_to_the_float64_sums(name):
    """One bright pixel in a corner or the middle of 37 x 21, 8 levels asked for: every level on the way down against plain float64
    sums over the same clamped indices (tests/bloom_float64.py).  All values are >= 0, so a sum's relative error is at most that of
    its worst operand plus one rounding: a level-i texel has behind it the bright pass (6 roundings, each relative to at most 2 m:
    12), the box (2 additions deep; x 0.25 is exact) and i down passes of two binomials, each 3 roundings deep ((b + d), x 4 exact,
    + (a + e), + 6 c): K_i = 14 + 6 i roundings, and the level's SUM inherits the bound of its texels."""
    rgb, p = ref.constructed_cases()[name]
    _, _, down, _ = ref.frame(rgb, p, want_levels=True)
    want = f64.bloom(rgb, p.threshold, p.knee, p.intensity, p.scatter, p.levels)
    assert len(down) == want["n"] == 6 and down[-1].shape == (1, 1, 3)
    for i, (got, exact) in enumerate(zip(down, want["levels"])):
        assert got.shape == exact.shape
        total = exact.sum(axis=(0, 1))
        assert (total > 0).all()
        assert (np.abs(got.astype(np.float64).sum(axis=(0, 1)) - total) <= (14 + 6 * i) * U * total).all(), (i, got.sum(axis=(0, 1)), total)
        # where the impulse cannot reach, the level is +0 to the bit (a clamped index that wandered would put mass there)
        assert np.array_equal(bits(got) == 0, exact == 0), i


# ---- hostile pixels ---------------------------------------------------------------------------------------------------------------------------
def test_a_nan_an_infinity_and_a_negative_pixel_do_not_spread():
    bad, clean, nan_at = ref.hostile()
    out, layer = ref.frame(bad, ref.params())
    clean_out, clean_layer = ref.frame(clean, ref.params())
    assert np.array_equal(bits(layer), bits(clean_layer))  # the layer is that of the frame with those channels as 0 / 2^20
    assert np.isfinite(layer).all()
    nan = np.isnan(out)
    assert nan.sum() == 1 and nan[nan_at][0]  # the NaN channel is the only NaN ...
    other = np.ones(out.shape, dtype=bool)
    other[6, 9, 0] = other[nan_at][0] = False
    assert np.isfinite(out[other]).all() and out[6, 9, 0] == np.inf  # ... the infinite channel stays itself, every other one is finite
    same = np.ones(out.shape[:2], dtype=bool)
    same[5, 6] = same[6, 9] = same[4, 5] = False
    assert np.array_equal(bits(out[same]), bits(clean_out[same]))


def test_denormals_are_arithmetic_like_any_other():
    """Channels of about 1e-39 with threshold 0 (knee 0): w = m, scale = 1, the bright pixel is the pixel, and the pyramid is sums of
    denormals — exact as integers of 2^-149 until they are scaled."""
    rgb, p = ref.constructed_cases()["denormals"]
    assert (rgb > 0).all() and (rgb < 2.0 ** -126).all()
    out, layer, down, _ = ref.frame(rgb, p, want_levels=True)
    assert (layer > 0).all() and (down[0] < 2.0 ** -126).all() and (out > rgb).all()
    want = f64.bloom(rgb, p.threshold, p.knee, p.intensity, p.scatter, p.levels)
    # level 0 is (b00 + b10 + b01 + b11) / 4 of exact integers of 2^-149: one rounding, of the quarter, half a unit at most
    assert (np.abs(down[0].astype(np.float64) - want["levels"][0]) <= 2.0 ** -150).all()


# ---- the level plan ---------------------------------------------------------------------------------------------------------------------------
PLANS = [  # (width, height, levels asked for) -> the sizes
    ((1, 1, 6), [(1, 1)]),
    ((1, 2, 6), [(1, 1)]),
    ((2, 1, 6), [(1, 1)]),
    ((3, 3, 6), [(2, 2), (1, 1)]),
    ((5, 3, 8), [(3, 2), (2, 1), (1, 1)]),
    ((67, 35, 6), [(34, 18), (17, 9), (9, 5), (5, 3), (3, 2), (2, 1)]),
    ((67, 35, 8), [(34, 18), (17, 9), (9, 5), (5, 3), (3, 2), (2, 1), (1, 1)]),
    ((32768, 1, 6), [(16384, 1), (8192, 1), (4096, 1), (2048, 1), (1024, 1), (512, 1)]),
    ((1, 32768, 8), [(1, 16384 >> i) for i in range(8)]),
    ((1920, 1080, 1), [(960, 540)]),
]


@pytest.mark.parametrize("asked,sizes", PLANS)
def test_the_level_plan(asked, sizes):
    width, height, levels = asked
    p = ref.params(levels=levels)
    plan = ref.plan(width, height, p)
    assert plan["sizes"] == sizes and plan["levels"] == len(sizes)
    assert plan["scratch_bytes"] == 12 * sum(w * h for w, h in sizes)
    assert plan["offsets"] == [3 * sum(w * h for w, h in sizes[:i]) for i in range(len(sizes))]
    assert f64.level_sizes(width, height, levels) == sizes  # (the float64 restatement's own rule agrees)
    norm, term = F32(0), F32(1)
    for _ in sizes:
        norm, term = F32(norm + term), F32(term * F32(p.scatter))
    assert plan["norm"] == norm and plan["gain"] == F32(F32(p.intensity) / norm)
    # rt_hip_bloom_plan (host-only) says the same
    assert rt_amd.renderer.bloom_plan(width, height, p) == {"levels": len(sizes), "last_width": sizes[-1][0], "last_height": sizes[-1][1], "scratch_bytes": plan["scratch_bytes"]}


def test_rt_hip_bloom_plan_refuses_by_name():
    for width, height in ((0, 5), (5, 0), (32769, 1)):
        with pytest.raises(capi.RtHipError) as refused:
            rt_amd.renderer.bloom_plan(width, height)
        assert refused.value.status == INVALID_ARGUMENT and f"frame {width}x{height}" in str(refused.value)
    with pytest.raises(capi.RtHipError) as refused:
        rt_amd.renderer.bloom_plan(8, 8, ref.params(levels=9))
    assert refused.value.status == INVALID_ARGUMENT and "levels" in str(refused.value) and "rt_hip_bloom_plan" in str(refused.value)
    assert capi.hip_lib().rt_hip_bloom_plan(8, 8, None, None) == INVALID_ARGUMENT


# ---- parameters -------------------------------------------------------------------------------------------------------------------------------
def test_the_defaults():
    assert ref.params().as_dict() == {"threshold": 1.0, "knee": 0.5, "intensity": F32(0.1), "scatter": F32(0.7), "levels": 6}
    assert rt_amd.renderer.bloom_default_params().as_dict() == ref.params().as_dict()
    assert ref.check(ref.params()) == (0, "")


NAN, INF = float("nan"), float("inf")
REFUSED = [
    ("threshold", [NAN, -1.0, INF, 2.0 ** 21, -INF]),
    ("knee", [NAN, -0.5, 2.0 ** -21, 1.5, INF]),  # (1.5: above the default threshold of 1)
    ("intensity", [NAN, -0.1, 1025.0, INF]),
    ("scatter", [NAN, -0.1, 1.0001, INF]),
    ("levels", [0, 9, 2 ** 31]),
]


@pytest.mark.parametrize("field,values", REFUSED)
def test_every_refusal_names_its_field(field, values):
    for value in values:
        status, message = ref.check(ref.params(**{field: value}))
        assert status == INVALID_ARGUMENT and message.startswith(f"rt_hip_bloom_params: {field} = "), (field, value, message)


def test_the_limits_themselves_are_accepted():
    for fields in (dict(threshold=0.0, knee=0.0), dict(threshold=2.0 ** 20, knee=2.0 ** 20), dict(knee=2.0 ** -20), dict(knee=1.0), dict(intensity=0.0), dict(intensity=1024.0), dict(scatter=0.0), dict(scatter=1.0), dict(levels=1),
                   dict(levels=8)):
        assert ref.check(ref.params(**fields)) == (0, ""), fields


# ---- the parser -------------------------------------------------------------------------------------------------------------------------------
def test_the_parser_accepts():
    accepted = {
        b"default": {},
        b"intensity=0.25": dict(intensity=0.25),
        b"levels=8": dict(levels=8),
        b"threshold=2,knee=1.5": dict(threshold=2.0, knee=1.5),
        b"scatter=1,levels=1,intensity=0,threshold=0,knee=0": dict(scatter=1.0, levels=1, intensity=0.0, threshold=0.0, knee=0.0),
        b"knee=.25": dict(knee=0.25),
        b"intensity=1e-1": dict(intensity=0.1),
    }
    for spec, fields in accepted.items():
        status, message, p = ref.from_spec(spec)
        assert status == 0 and message == "" and p.as_dict() == ref.params(**fields).as_dict(), spec
        assert rt_amd.renderer.bloom_from_spec(spec.decode()).as_dict() == p.as_dict()


def test_the_parser_refuses_and_quotes_the_text():
    refused = [b"", b"bloom", b"defaults", b"intensity", b"intensity=", b"=1", b"intensity=0.1,", b",intensity=0.1", b"intensity=0.1;knee=0.2", b"intensity=0.1,intensity=0.2", b"glow=1", b"Intensity=1", b"intensity= 1",
               b"intensity=+1", b"intensity=-1", b"intensity=nan", b"intensity=inf", b"intensity=0x1p0", b"intensity=1e99", b"levels=2.5", b"levels=0", b"levels=9", b"levels=1e3", b"knee=2", b"scatter=1.5",
               b"threshold=1,knee=0.5,intensity=0.1,scatter=0.7,levels=6,levels=6", b"intensity=" + b"1" * 40]
    for spec in refused:
        sentinel = ref.params(levels=3)
        status, message, _ = ref.from_spec(spec)
        assert status == INVALID_ARGUMENT and message.startswith("rt_hip_bloom_from_spec: '" + spec.decode()[:64]), (spec, message)
        assert capi.hip_lib().rt_hip_bloom_from_spec(spec, sentinel) == INVALID_ARGUMENT and sentinel.levels == 3  # (untouched)
        assert capi.hip_lib().rt_hip_last_error().decode() == message
    long = b"x" * 300
    status, message, _ = ref.from_spec(long)
    assert status == INVALID_ARGUMENT and "'" + "x" * 64 + "...'" in message
    assert "knee" in ref.from_spec(b"knee=2")[1] and "levels" in ref.from_spec(b"levels=9")[1]  # (a refused value names its field too)
    assert capi.hip_lib().rt_hip_bloom_from_spec(None, ref.params()) == INVALID_ARGUMENT
    assert capi.hip_lib().rt_hip_bloom_default_params(None) == INVALID_ARGUMENT
