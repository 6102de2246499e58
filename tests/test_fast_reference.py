"""The conditions the per-pixel rule of RT_HIP_FLAG_FAST's builds (tests/fast_reference.py) must meet FROM THE REFERENCE SIDE ALONE, on the
CPU, for every case of tests/fast_cases.py — before any GPU frame is held to it (tests/test_gpu_fast_builds.py):

  * the float32 oracle's frame has no pixel beyond the allowance, and neither has any of 16 stand-ins for a FAST frame (single perturbed
    runs at S and S / 2 ulps, seeds disjoint from the ensemble's): what is legitimately different passes;
  * teeth: tight pixels (allowance <= 1e-4 * scale) are at least half the frame and at least half of the pixels in which a sample
    bounces, and two deliberately wrong tracers — the unit-vector draw scaled by 1.001; each pixel's last sample drawn from the next
    sample index's stream — each put at least 1 % of the frame's pixels beyond the allowance;
  * a tight pixel's packed channels are within 1 of pack(sqrt(base));
  * every case's frame takes the build the table names, and together the cases reach every fast instantiation but streamed-dense."""
import numpy as np
import pytest

from oracle import binding as oracle
from tests import fast_cases as cases
from tests import fast_reference as ref

NAMES = [case.name for case in cases.CASES]


@pytest.mark.parametrize("name", NAMES)
def test_what_may_differ_passes_and_what_is_wrong_does_not(name):
    case = cases.BY_NAME[name]
    rule = cases.reference(name)
    _, oracle_mean, _ = cases.oracle_frame(name)
    stand_ins, wrong_a, wrong_b = cases.check_frames(name)
    pixels = rule.tight.size
    oracle_excess = rule.excess(oracle_mean)
    stand_in_excess = np.stack([rule.excess(frame) for frame in stand_ins])
    beyond_a, beyond_b = int((rule.excess(wrong_a) > 1.0).sum()), int((rule.excess(wrong_b) > 1.0).sum())
    tight, tight_of_bouncing = float(rule.tight.mean()), float(rule.tight[rule.bounced].mean())
    print(f"{name}: {case.spp} samples x {case.bounces} bounces: oracle worst diff / allowance {oracle_excess.max():.3f}, stand-ins {stand_in_excess.max():.3f}; tight {tight:.2f} of the frame, {tight_of_bouncing:.2f} of the "
          f"{int(rule.bounced.sum())} bouncing pixels; wrong (a) {beyond_a}, (b) {beyond_b} of {pixels} pixels beyond")
    assert (oracle_excess <= 1.0).all(), f"the float32 oracle: {int((oracle_excess > 1.0).sum())} pixels beyond the allowance, the first at {tuple(np.argwhere(oracle_excess > 1.0)[0])}: {oracle_excess.max():.2f} times"
    assert (stand_in_excess <= 1.0).all(), f"stand-ins: {int((stand_in_excess > 1.0).sum())} pixels beyond the allowance, (run, y, x) = {tuple(np.argwhere(stand_in_excess > 1.0)[0])}: {stand_in_excess.max():.2f} times"
    assert tight >= 0.5 and tight_of_bouncing >= 0.5
    assert beyond_a >= 0.01 * pixels and beyond_b >= 0.01 * pixels


@pytest.mark.parametrize("name", NAMES)
def test_a_tight_pixels_packed_channels_differ_by_at_most_one(name):
    """A channel is packed as trunc(clamp01(sqrt(c)) * 255.99999).  In a tight pixel |c' - c| <= 1e-4 * scale, and every channel of a
    case's pixel is at least CHANNEL_RATIO = 0.5^7 of its largest, `scale` <= 1 (tests/fast_cases.py: albedo ratios, bounce limit, sky;
    asserted here) — so for c > 0:
        |sqrt(c') - sqrt(c)| = |c' - c| / (sqrt(c') + sqrt(c)) <= 1e-4 * scale / (2 * sqrt((CHANNEL_RATIO - 1e-4) * scale)) <= 5.7e-4 * sqrt(scale)
    which is 0.146 of a level at scale = 1: less than one level, so the truncated values differ by at most 1.  (A black pixel — every path
    of it ends black — is black in base and frame alike or it is not tight.)  The oracle's frames are held to it."""
    case = cases.BY_NAME[name]
    rule = cases.reference(name)
    lit = rule.base.max(axis=-1) > 0.0
    assert (rule.base.min(axis=-1)[lit] >= cases.CHANNEL_RATIO * rule.scale[lit] * (1 - 1e-12)).all() and rule.scale.max() <= 1.0 and case.bounces <= cases.MAX_BOUNCES
    assert 255.99999 * 1e-4 / (2.0 * np.sqrt(cases.CHANNEL_RATIO - 1e-4)) < 1.0
    rgba, _, _ = cases.oracle_frame(name)
    levels = np.abs(ref.channels(rgba) - ref.pack(rule.base)).max(axis=-1)
    assert (levels[rule.tight] <= 1).all(), (name, int((levels[rule.tight] > 1).sum()))
    assert ((rgba & 0xFF) == 0xFF).all()


def plans_of(case):
    """every (variant, host_frame, local rows) the GPU tests render the case with"""
    for variant in case.variants:
        yield variant, 1, None
        if case.hbm:
            yield variant, 0, None
        if case.stripes:
            for rank in range(3):
                yield variant, 0, len(cases.stripe_rows(case.height, rank))


@pytest.mark.parametrize("name", NAMES)
def test_the_cases_frame_takes_the_build_the_table_names(name):
    case = cases.BY_NAME[name]
    for variant, host, rows in plans_of(case):
        cases.assert_plan(case, variant, host, rows)
    if case.sweep == "chunks":  # the sweep is there for the tile sizes and the two ways a tile is folded
        assert {variant.pixels_log2 for variant in case.variants} <= {2, 3, 4, 5}
    if case.scene[2] == "eye":
        assert pod_noise(case)
    if case.stripes:  # a rank's frame holds its rows top down: the rows of the whole frame's rule the GPU test holds it to
        whole = cases.oracle_frame(name)[0]
        for rank in range(3):
            part, _, _ = oracle.render(cases.pod_of(case), case.width, case.height, seed=case.seed, partition=(rank, 3, 5), want_rgb=False)
            assert np.array_equal(part, whole[cases.stripe_rows(case.height, rank)])


def pod_noise(case):
    """the eye cases' matrix carries rounding noise in the last row's x / y terms: w varies over the frame"""
    matrix = cases.pod_of(case).inverse_view_projection
    return matrix[12] != 0.0 or matrix[13] != 0.0


def test_the_cases_reach_every_fast_instantiation_but_streamed_dense(capsys):
    """DESIGN.md counts 116 kernels in the fast build: 26 (spheres, planes) pairs x pinhole / eye x whole / sub-chunk items, the three
    resident forms x 2, tiled, streamed and streamed-dense x 2.  Listed here: which of them the table's frames take, by the plan dump.
    streamed-dense is named only for launches of 4M samples and more (launch_plan.cpp): no frame of this size can ask for it."""
    reached = {}
    for case in cases.CASES:
        for variant, host, rows in plans_of(case):
            p = cases.assert_plan(case, variant, host, rows)
            assert p["scan"] != cases.SCAN_STREAMED_DENSE
            reached.setdefault(cases.instantiation(variant), set()).add((p["chunks"], p["pixels_log2"], "HBM" if not host else "page-locked"))
    with capsys.disabled():
        print(f"\nfast instantiations reached by tests/fast_cases.py ({len(reached)} of 116): (K, pixels_log2, destination)")
        for build in sorted(reached):
            print(f"  {build}: " + ", ".join(f"({k}, {log2}, {where})" for k, log2, where in sorted(reached[build])))
    expected = [f"scalar-register ({s} spheres, {p} planes), {camera}, {items}" for s, p in cases.PAIRS for camera in ("pinhole", "eye") for items in ("whole", "HALF")]
    expected += [f"resident ({form}), {items}" for form in ("LDS scan, pinhole", "LDS scan, general camera", "scalar-load scan") for items in ("whole", "HALF")]
    expected += [f"{kernel}, {items}" for kernel in ("tiled", "streamed") for items in ("whole", "HALF")]
    assert len(cases.PAIRS) == 26 and len(expected) == 114
    assert sorted(reached) == sorted(expected), sorted(set(expected) ^ set(reached))
    # the chunk sweep: K = 2 ... 33, every tile size from 32 pixels down to 4 in both kernels, HALF up to K = 16
    swept = {(v.kernel, v.halves, v.chunks, v.pixels_log2) for case in cases.of_sweep("chunks") for v in case.variants}
    for kernel in ("small", "resident"):
        assert {(k, log2) for name, half, k, log2 in swept if name == kernel and half} == {(2, 4), (3, 3), (5, 2), (9, 2), (16, 2)}
        assert {(k, log2) for name, half, k, log2 in swept if name == kernel and not half} == {(2, 5), (3, 4), (5, 3), (9, 2), (16, 2), (17, 2), (33, 2)}
