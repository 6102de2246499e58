"""Guided upsampling's float32 restatement (tests/upsample_reference.py: rt_amd/csrc/upsample_rules.hpp, serially) against a SECOND
reading of DESIGN.md §3.14 in float64 numpy (tests/upsample_float64.py): `upsample::tap_weight` is a hand copy of `denoise::tap_weight`
minus two terms, the kernel and the restatement compile the same text, and tests/test_upsample_rules.py holds the pixel rule only where
every guided term is exactly 1 — so a slip in that copy is wrong on both sides and passes everything else.  Not here.

The bound.  Per pixel and channel  |float32 − float64| ≤ K · u · scale · (1 + K u) + A,  u = 2⁻²⁴ (one rounding's relative error),
`scale` the pixel's magnitude in the float64 reading: the same quotient over |c|.  K counts the roundings on the longest chain from the
inputs to a pixel, in the order §3.14 fixes, for the case's s = normal_squarings.  Every sum below has non-negative terms (weights; the
products of a dot of two of tests/upsample_reference.random_guide's normals, whose components are never negative), so an operand's
relative error is at most that of its worst term plus the adds it passes through:

  b = bx · by           bx and by are one correctly rounded quotient of two exact integers each, the product one more: 3
  normal term           the dot: a product and two adds, 3; max(0, ·) none; a squaring doubles the relative error and rounds once,
                        e → 2 e + 1, s times from 3:  4 · 2^s − 1
  depth term            Δz 1 (relative to itself), sigma_depth · max z 1, the quotient 1: 3; squared 2 · 3 + 1 = 7; 1 + · at most 7 and a
                        rounding: 8; the reciprocal: 9
  albedo term           each Δa 1, squared 3, two adds 5; sigma_albedo² 1 and the quotient 1: 7; 1 + ·: 8; the reciprocal: 9
  the weight            b, then × normal, × depth, × albedo, a rounding each:  E(s) = 3 + (4 · 2^s − 1) + 1 + (9 + 1) + (9 + 1) = 4 · 2^s + 23
  sw                    four terms, 0 + w exact, three adds:  E + 3
  Σ w c                 w · c one rounding, three adds:  E + 4, relative to Σ w |c| (the colours have both signs)
  the quotient          one rounding:  |δ out| ≤ ((E + 4) + (E + 3) + 1) · u · Σ w |c| / sw

  K(s) = 2 E(s) + 8 = 8 · 2^s + 54:  62, 118 and 2102 for s = 0, 3 and 8.   An orphan's bilinear mean is the same chain with b alone
  for a weight (E = 3):  K = 14.

K is the sum of worst cases and is not tuned.  It is far from sharp, and the recorded ratios say so (profiles/r32/upsample_float64.txt):
the weight's error is common to Σ w c and sw and cancels in their quotient, while the bound adds it twice; and a squaring chain
reaches 2^s times its input's error only if every rounding on the way falls the same side.  What a slip in the rule does is of another
order: an unsquared sigma, a term over the wrong depth or a normal term on sky moves pixels by 10⁻² of their scale and more.

Underflow (A).  Float32 underflows where float64 does not: 0.6 and 0.64, two of the dots random_guide's normals have, squared eight
times are 2⁻¹⁸⁹ and 2⁻¹⁶⁵ — 0 or a denormal in float32.  The bound CARRIES AN ABSOLUTE TERM for it rather than restricting the
normals: a weight that left the normal range is wrong by at most 2⁻¹⁴⁹; a guided pixel has sw ≥ min_weight ≥ 2⁻²⁰ in every case
here and |c| < 2, so four such taps move a channel by at most 4 · 2⁻¹⁴⁹ · 2 · 2²⁰ = 2⁻¹²⁶.  A = 2⁻¹²⁰.

The one discontinuous selection is guided-or-orphan at sw ≥ min_weight.  A pixel whose float64 sw lies within sw's own bound,
(E + 3) · u · sw, of min_weight may take the other branch in float32: those are EXCLUDED from the comparison of the values, counted, and
their share must be at most 1 % of the case's pixels.  The restatement reports the orphan COUNT, not a mask (its ABI is the device's):
outside the excluded set the masks are held equal through the values — a pixel on the other branch holds the other mean — and the count
must be the float64 reading's, give or take the excluded pixels (exactly, where none is excluded).  Every other selection (max(0, ·),
max z, the sky rules on exact ids, finiteness on exact bits) is continuous in its operands or decided by exact inputs.

The non-finite rules carry no tolerance: a NaN or infinite tap has weight 0 and colour 0 in both readings, at the same positions, and a
neighbourhood with no usable tap is (0, 0, 0) and an orphan in both."""
import numpy as np
import pytest

from tests import upsample_float64 as f64
from tests import upsample_reference as ref

F32 = np.float32
U = 2.0**-24
A = 2.0**-120


def E(squarings: int) -> int:
    return 4 * 2**squarings + 23


def K(squarings: int) -> int:
    return 2 * E(squarings) + 8


K_ORPHAN = 2 * 3 + 8
TIGHT = dict(sigma_albedo=0.01, sigma_depth=0.001, min_weight=0.5)
WIDE = dict(sigma_albedo=10.0, sigma_depth=10.0, min_weight=1e-6)

CASES = {  # name -> (W, H, w, h, seed, share of sky, poisoned, parameters); the size pairs are tests/test_gpu_upsample.py's SHAPES
    "1x1 from 1x1": (1, 1, 1, 1, 1, 0.25, False, {}),
    "2x2 from 1x1": (2, 2, 1, 1, 2, 0.25, False, {}),
    "17x17 from 9x9": (17, 17, 9, 9, 3, 0.25, False, {}),
    "33x5 from 33x5 (w = W), poisoned": (33, 5, 33, 5, 4, 0.25, True, {}),
    "37x3 from 1x1": (37, 3, 1, 1, 5, 0.0, False, {}),
    "70x41 from 18x11, defaults (3 squarings), poisoned": (70, 41, 18, 11, 6, 0.25, True, {}),
    "70x41 from 18x11, 0 squarings, wide, min_weight 1": (70, 41, 18, 11, 7, 0.25, False, dict(normal_squarings=0, sigma_albedo=5.0, sigma_depth=5.0, min_weight=1.0)),
    "70x41 from 18x11, 0 squarings, wide": (70, 41, 18, 11, 8, 0.25, False, dict(normal_squarings=0, **WIDE)),
    "70x41 from 18x11, 8 squarings, tight": (70, 41, 18, 11, 9, 0.25, False, dict(normal_squarings=8, **TIGHT)),
    "70x41 from 18x11, 8 squarings, wide": (70, 41, 18, 11, 10, 0.25, True, dict(normal_squarings=8, **WIDE)),
    "70x41 from 18x11, sky only": (70, 41, 18, 11, 11, 1.0, False, {}),
    "70x41 from 18x11, hits only": (70, 41, 18, 11, 12, 0.0, False, {}),
}


def inputs(name):
    W, H, w, h, seed, sky_share, poisoned, fields = CASES[name]
    rng = np.random.default_rng(seed)
    low = rng.uniform(-0.2, 1.5, size=(h, w, 3)).astype(F32)
    guide_low, guide_full = ref.random_guide(rng, h, w, sky_share), ref.random_guide(rng, H, W, sky_share)
    if poisoned:
        low[h // 2, w // 3, 1] = np.nan
        low[h - 1, w - 1, 2] = np.inf
    return low, guide_low, guide_full, ref.params(**fields)


def float64_of(low, guide_low, guide_full, p):
    """(the parameters as the float32 values they are: both readings start from the same numbers)"""
    return f64.frame(low, guide_low, guide_full, p.normal_squarings, float(p.sigma_albedo), float(p.sigma_depth), float(p.min_weight))


@pytest.mark.parametrize("name", list(CASES))
def test_the_float32_restatement_lies_within_the_counted_roundings_of_the_float64_reading(name):
    low, guide_low, guide_full, p = inputs(name)
    got, _, got_orphans = ref.frame(low, guide_low, guide_full, p)
    want = float64_of(low, guide_low, guide_full, p)
    s, pixels = p.normal_squarings, want["sw"].size
    assert p.min_weight >= 2.0**-20  # (what A was worked out for)
    # the sliver about the threshold: left out of the values, counted, at most 1 %
    excluded = np.abs(want["sw"] - float(p.min_weight)) <= (E(s) + 3) * U * want["sw"] * (1 + K(s) * U)
    assert excluded.mean() <= 0.01, f"{name}: {excluded.sum()} of {pixels} pixels lie within sw's bound of min_weight"
    certain = int((want["orphan"] & ~excluded).sum())
    assert certain <= got_orphans <= certain + int(excluded.sum()), (name, got_orphans, want["orphans"], int(excluded.sum()))
    k = np.where(want["orphan"], K_ORPHAN, K(s))[..., None]
    bound = k * U * want["scale"] * (1 + k * U) + A
    error = np.abs(got.astype(np.float64) - want["out"])
    ratio = np.where(excluded[..., None], 0.0, error / bound)
    worst = {branch: float(ratio[at].max()) if at.any() else 0.0 for branch, at in (("guided", ~want["orphan"]), ("orphans", want["orphan"]))}
    print(f"{name}: s = {s}, K = {K(s)} (orphans {K_ORPHAN}); worst error / bound: guided {worst['guided']:.4f}, orphans {worst['orphans']:.4f}; "
          f"orphans {got_orphans} of {pixels} (float64: {want['orphans']}); excluded {int(excluded.sum())} ({100.0 * excluded.mean():.2f} %)")
    assert np.isfinite(got).all() and np.isfinite(want["out"]).all()  # (nothing non-finite comes out of either reading)
    assert (ratio <= 1.0).all(), (name, worst, np.argwhere(ratio > 1.0)[:4].tolist())


def test_the_cases_meet_both_branches_all_three_squaring_counts_and_every_kind_of_frame():
    seen = {name: float64_of(*inputs(name)) for name in CASES}
    assert {inputs(name)[3].normal_squarings for name in CASES} == {0, 3, 8}
    assert any(r["orphan"].any() and not r["orphan"].all() for r in seen.values())
    assert not seen["70x41 from 18x11, sky only"]["orphan"].any()  # sky against sky: b alone, and Σ b = 1
    assert seen["70x41 from 18x11, 0 squarings, wide, min_weight 1"]["orphan"].mean() > 0.5  # (a threshold that makes many orphans)
    # the weights matter: the tight and the wide reading of one frame differ by far more than any bound here
    low, guide_low, guide_full, p = inputs("70x41 from 18x11, 8 squarings, tight")
    other = f64.frame(low, guide_low, guide_full, 8, 10.0, 10.0, 1e-6)
    assert np.abs(other["out"] - seen["70x41 from 18x11, 8 squarings, tight"]["out"]).max() > 0.1


def test_a_slip_in_the_copied_weight_would_not_pass():
    """What the bound is for: the three slips a hand copy invites, made in the float64 reading (the float32 text is the product's),
    each leave the bound by orders of magnitude on the mixed default case."""
    name = "70x41 from 18x11, defaults (3 squarings), poisoned"
    low, guide_low, guide_full, p = inputs(name)
    got = ref.frame(low, guide_low, guide_full, p)[0].astype(np.float64)
    honest = float64_of(low, guide_low, guide_full, p)
    bound = K(p.normal_squarings) * U * honest["scale"] * 1.001 + A
    slips = {
        "sigma_albedo unsquared": f64.frame(low, guide_low, guide_full, p.normal_squarings, float(p.sigma_albedo) ** 0.5, float(p.sigma_depth), float(p.min_weight)),
        "one squaring short": f64.frame(low, guide_low, guide_full, p.normal_squarings - 1, float(p.sigma_albedo), float(p.sigma_depth), float(p.min_weight)),
        "sigma_depth doubled": f64.frame(low, guide_low, guide_full, p.normal_squarings, float(p.sigma_albedo), 2.0 * float(p.sigma_depth), float(p.min_weight)),
    }
    for what, slipped in slips.items():
        same_branch = slipped["orphan"] == honest["orphan"]
        worst = (np.abs(got - slipped["out"]) / bound)[same_branch].max()
        print(f"{what}: worst error / bound = {worst:.0f}")
        assert worst > 100.0, what


def test_the_non_finite_rules_agree_exactly():
    """w = W: pixel x sits on low pixel x, its other taps have b = 0.  Over a NaN or an infinite low pixel no tap is usable and Σ b is 0:
    (0, 0, 0) and an orphan, in both readings, at the same positions; and a frame whose every low pixel is bad is black and all orphans."""
    rng = np.random.default_rng(40)
    W, H = 33, 5
    low = rng.uniform(0.1, 1.0, size=(H, W, 3)).astype(F32)
    guide = ref.hit_guide(H, W)
    bad = [(2, 11, 1, np.nan), (4, 32, 2, np.inf), (0, 0, 0, -np.inf)]
    for y, x, channel, value in bad:
        low[y, x, channel] = value
    got, _, got_orphans = ref.frame(low, guide, guide, None)
    p = ref.params()
    want = float64_of(low, guide, guide, p)
    at = np.zeros((H, W), dtype=bool)
    for y, x, _, _ in bad:
        at[y, x] = True
    assert np.array_equal(want["orphan"], at) and got_orphans == want["orphans"] == 3
    assert not got[at].view(np.uint32).any() and not want["out"][at].any()
    assert np.array_equal(got[~at].astype(np.float64), want["out"][~at])  # (one tap of weight 1 on one surface: the low pixel itself)
    low[:] = np.nan
    got, _, got_orphans = ref.frame(low, guide, guide, None)
    want = float64_of(low, guide, guide, p)
    assert got_orphans == want["orphans"] == W * H and not got.view(np.uint32).any() and not want["out"].any()
