"""Bloom's float32 restatement (tests/bloom_reference.py: rt_amd/csrc/bloom_rules.hpp, serially) against a SECOND restatement in float64
numpy written from DESIGN.md §3.16's text alone (tests/bloom_float64.py): another author's reading of the same contract — whole-image
index arrays, numpy's own summation order — so a misread clamp, tap weight or level rule in the header does not pass for the contract.

The bound.  Per pixel and channel  |float32 - float64| <= K x 2^-24 x scale,  where `scale` is the pixel's MAGNITUDE in the float64
restatement: the same filters over the sanitised channels instead of the bright ones, plus |in| for the frame.  Everything behind the
bright pass is a sum with non-negative weights of non-negative values, so an operand's relative error is at most that of its worst
input plus one rounding, and `scale` bounds every operand on the way.  K counts the roundings on the LONGEST chain to a pixel for the
case's level count L (2^-24 = half an ulp of 1: one rounding's relative error):

  bright pass    6 roundings: threshold - knee; m - that; rq x rq; / (4 knee) [or m - threshold alone]; w / m; c x scale.  Each is
                 relative to its own result, which is at most 2 m wherever w > 0 (the knee engages at m >= threshold - knee >= threshold / 2
                 or the difference threshold - knee is exact), and scale <= 1 carries it to the channel: 12
  prefilter      (b00 + b10), + (b01 + b11); x 0.25 is exact: 2
  down, a level  two binomials, each 3 deep: (b + d), x 4 exact, + (a + e), + 6 c (6 c rounds, but lies beside the chain); x 1/256 exact: 6
  up, a level    the tent is two tent2, each 0.75 x near (x 0.25 is exact) and a sum: 4; scatter x tent, + level: 6
  composite      the tent: 4; gain x layer; + in: 6
  gain           norm is L - 1 sums and L - 1 products deep at most (the last term's chain), the quotient one more: 2 L - 1

  K(L) = 12 + 2 + 6 (L - 1) + 6 (L - 1) + 6 + (2 L - 1) = 14 L + 7.

No selection is excluded: every selection in the contract (the sanitising, max of the channels, the clamp of rq, max(soft, m - threshold),
m > 0) is continuous in its operands, so the two restatements taking different branches at a tie changes nothing beyond the roundings
counted.  The share of pixels left out is therefore 0, asserted below against the 1 % the contract allows."""
import numpy as np
import pytest

from tests import bloom_float64 as f64
from tests import bloom_reference as ref

U = 2.0 ** -24


def K(levels: int) -> int:
    return 14 * levels + 7


CASES = {  # name -> (height, width, seed, parameters)
    "defaults 37x21": (21, 37, 11, {}),
    "defaults 67x35": (35, 67, 12, {}),
    "eight levels 67x35": (35, 67, 13, dict(levels=8)),
    "one level 67x35": (35, 67, 14, dict(levels=1)),
    "hard knee": (21, 37, 15, dict(knee=0.0)),
    "knee up to the threshold": (21, 37, 16, dict(threshold=0.75, knee=0.75)),
    "wide and strong": (35, 67, 17, dict(scatter=1.0, intensity=8.0, levels=8)),
    "tight": (21, 37, 18, dict(scatter=0.0)),
    "threshold 0": (21, 37, 19, dict(threshold=0.0, knee=0.0, intensity=1.0)),
    "one row": (1, 300, 20, dict(levels=8)),
    "one column": (300, 1, 21, dict(levels=8)),
    "1x1": (1, 1, 22, {}),
}


@pytest.mark.parametrize("name", list(CASES))
def test_the_float32_restatement_lies_within_the_counted_roundings_of_the_float64_one(name):
    height, width, seed, fields = CASES[name]
    p = ref.params(**fields)
    rgb = ref.noise(height, width, seed=seed)
    out, layer, down, _ = ref.frame(rgb, p, want_levels=True)
    want = f64.bloom(rgb, p.threshold, p.knee, p.intensity, p.scatter, p.levels)
    L = want["n"]
    assert L == len(down) == ref.plan(width, height, p)["levels"]
    assert [l.shape for l in down] == [l.shape for l in want["levels"]]
    excluded = np.zeros((height, width), dtype=bool)  # (no tie is excluded: see above)
    assert excluded.mean() <= 0.01
    for what, got, exact, scale in (("layer", layer, want["layer"], want["layer_scale"]), ("frame", out, want["out"], want["out_scale"])):
        error = np.abs(got.astype(np.float64) - exact)
        bound = K(L) * U * scale
        worst = (error / np.maximum(bound, 1e-300)).max()
        print(f"{name}: {what}: L = {L}, K = {K(L)}, worst error / bound = {worst:.3f}")
        assert (error[~excluded] <= bound[~excluded]).all(), (what, worst)
    assert (want["layer"] > 0).any() or name == "1x1"  # (the case glows at all)


def test_hostile_pixels_too():
    bad, _, nan_at = ref.hostile()
    p = ref.params()
    out, layer = ref.frame(bad, p)
    want = f64.bloom(bad, p.threshold, p.knee, p.intensity, p.scatter, p.levels)
    assert (np.abs(layer.astype(np.float64) - want["layer"]) <= K(want["n"]) * U * want["layer_scale"]).all()
    finite = np.isfinite(bad)
    with np.errstate(invalid="ignore"):  # (inf - inf at the infinite channel, which `finite` leaves out)
        error = np.abs(out.astype(np.float64) - want["out"])
    assert (error[finite] <= (K(want["n"]) * U * want["out_scale"])[finite]).all()
    assert np.array_equal(np.isnan(out), np.isnan(want["out"])) and np.isnan(out).sum() == 1 and np.isnan(out[nan_at][0])
