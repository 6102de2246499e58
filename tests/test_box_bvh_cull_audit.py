"""The cull of RT_HIP_FLAG_BOX_BVH (rt_amd/csrc/box_bvh_scan.hpp) audited against the box contract's CPU restatement, on the host (no GPU),
in the manner of tests/test_bvh_cull_audit.py.

tests/native/box_reference.cpp's closest hit is the linear scan's answer bit for bit.  For a ray it answers with tree box i at
distance t, the traversal returns the same answer, whatever order it visits nodes in, if and only if it never skips a node on the
way from the root to i's leaf.  This checks exactly that with a numpy binary32 restatement of enter_node holding best.t = t — the
tightest it can be while box i is still to be found — and, for one random tree box per ray whether hit or not, the lemma the cull
rests on: the node's computed tmin is <= the box's and its tmax >= the box's, with no pad.  Scenes from 2^-60 to 2^38, origins on
faces, on edges, inside nested boxes and far away, directions with tiny components whose reciprocals stay finite; and the gate:
lanes with a zero, subnormal or overflowing-reciprocal component, or a non-finite origin, are classified for the linear scan.
The GPU side, the compiled traversal on the same scenes and rays, is tests/test_gpu_box_bvh.py."""
import numpy as np
import pytest

from tests import box_bvh_cases as cases

SCALES = [-60, -40, -20, -6, 0, 7, 20, 38]


def scale_case(exponent, rays=6000):
    """The scene and rays of one scale: the same bytes wherever and whenever they are asked for."""
    rng = np.random.default_rng([11, exponent + 100])
    k = 2.0**exponent
    rows = cases.scaled(cases.random_boxes(rng, 400, nested=6), k)
    origins, dirs = cases.rays_at(rows, rng, rays, scale=k)
    # a third of the directions get one tiny component whose reciprocal is huge but finite (2^-100 .. 2^-20)
    tiny = rng.integers(0, 3, rays) == 0
    axis = rng.integers(0, 3, rays)
    dirs[tiny, axis[tiny]] = (np.sign(rng.normal(size=int(tiny.sum()))) * 2.0 ** rng.uniform(-100, -20, int(tiny.sum()))).astype(np.float32)
    return rows, origins, dirs, rng


@pytest.mark.parametrize("exponent", SCALES)
def test_no_node_on_the_way_to_the_answer_is_skipped(exponent):
    rows, origins, dirs, rng = scale_case(exponent)
    found = cases.audit_cull(rows, origins, dirs, rng)
    print(f"scale 2^{exponent}: {found}")
    assert found["taken"] == found["rays"], "no ray of this set is built for the fall-back"
    # so that the audit cannot pass by looking at nothing (the 0.001 rule is absolute: tiny scenes answer only from outside it)
    assert found["answered"] >= (0.25 if exponent >= -6 else 0.02) * found["rays"], found
    assert found["skipped"] == 0, found.get("first")
    assert found["lemma_broken"] == 0


def test_the_depth_24_chain_and_identical_boxes():
    rng = np.random.default_rng(5)
    for rows in (cases.chain_boxes(0, 1.0), cases.chain_boxes(2, -1.0), np.array([(1, 2, 3, 0.5, 0.25, 0.125, 0)] * 64, dtype=np.float64)):
        origins, dirs = cases.rays_at(rows, rng, 4000)
        found = cases.audit_cull(rows, origins, dirs, rng)
        print(found)
        assert found["answered"] > 400 and found["skipped"] == 0 and found["lemma_broken"] == 0, found


def test_boxes_with_lo_above_hi():
    rng = np.random.default_rng(6)
    rows = cases.random_boxes(rng, 300)
    rows[::2, 3:6] *= -1  # the uploaded pair has lo > hi: hits_box answers as for the swapped box, and so must the node test
    origins, dirs = cases.rays_at(rows, rng, 6000)
    found = cases.audit_cull(rows, origins, dirs, rng)
    assert found["answered"] > 1500 and found["skipped"] == 0 and found["lemma_broken"] == 0, found


def test_degenerate_lanes_are_classified_for_the_fall_back():
    rng = np.random.default_rng(7)
    origins = rng.uniform(-3, 3, (5000, 3)).astype(np.float32)
    dirs = cases.degenerate_directions(rng, 5000)
    takes = cases.gate_takes(origins, dirs)
    inv = cases.reciprocal(dirs)
    zero = (dirs == 0).any(axis=1)
    overflowing = np.isinf(inv).any(axis=1)
    assert zero.sum() > 500 and (overflowing & ~zero).sum() > 200 and takes.sum() > 500
    assert not takes[zero].any(), "a lane with a zero component (either sign) must take the linear scan"
    assert not takes[overflowing].any(), "a lane whose reciprocal overflows (a subnormal component) must take the linear scan"
    assert takes[~overflowing].all()
    # the tiniest components the gate admits: the reciprocal is finite, nothing becomes a NaN, the lemma holds
    rows = cases.random_boxes(rng, 200, nested=4)
    found = cases.audit_cull(rows, origins[takes], dirs[takes], rng)
    assert found["skipped"] == 0 and found["lemma_broken"] == 0
    # non-finite origins and directions
    for bad in (np.inf, -np.inf, np.nan):
        o = origins[:6].copy()
        o[np.arange(6), np.arange(6) % 3] = bad
        assert not cases.gate_takes(o, np.tile(np.float32([0.6, 0.0, 0.8]) + np.float32([0, 0.5, 0]), (6, 1))).any()
        d = np.tile(np.float32([0.6, 0.5, 0.8]), (6, 1))
        d[np.arange(6), np.arange(6) % 3] = bad
        assert not cases.gate_takes(origins[:6], d).any()  # (1 / inf = 0: the reciprocal is finite and the gate still closes)


def test_a_difference_that_overflows_stays_ordered():
    """Corners and origins near the end of binary32: lo - o overflows to an infinity, which a finite non-zero reciprocal keeps in order."""
    rng = np.random.default_rng(8)
    rows = cases.scaled(cases.random_boxes(rng, 100, spread=1.0, e_lo=0.01, e_hi=0.2), 2.0**126)
    origins, dirs = cases.rays_at(rows, rng, 3000, scale=2.0**126)
    origins = np.where(rng.integers(0, 2, origins.shape) == 0, origins, -origins).astype(np.float32)
    found = cases.audit_cull(rows, origins, dirs, rng)
    # (the far origins of this set overflow binary32 and close the gate: they are the fall-back's)
    assert found["taken"] > 0.5 * found["rays"] and found["answered"] > 100 and found["skipped"] == 0 and found["lemma_broken"] == 0, found
