"""The cull bound of RT_HIP_FLAG_BVH (rt_amd/csrc/bvh_scan.hpp) audited against the oracle, on the host (no GPU).

The oracle's closest hit is the linear scan's answer bit for bit (tests/test_oracle_kat.py).  For a ray it answers with tree
sphere i at distance t, the traversal returns the same answer, whatever order it visits nodes in, if and only if it never
culls a box on the way from the root to i's leaf.  This checks exactly that, per regime of tests/bvh_cases.py, with a numpy
binary32 restatement of enter_box whose pad is at most the device's (bvh_cases.audit_cull); no sphere arithmetic is restated.
The GPU side, the compiled traversal on the same scenes and rays, is tests/test_gpu_bvh.py.

Also here: the builder driven to its depth limit and the always list driven to its cap.

`python -m tests.test_bvh_cull_audit` prints the table of profiles/r07/bvh_cull_audit.txt."""
import numpy as np
import pytest

from rt_amd.renderer import bvh_build
from tests import bvh_cases
from tests.bvh_cases import STACK_DEPTH, check_tree, sphere_scene
from tests.test_bvh_build import build_twice, header_constant


def audit(name):
    total = {"rays": 0, "answered": 0, "excluded": 0, "culled": 0, "slack": np.inf, "cases": []}
    for label, rows, origins, dirs in bvh_cases.regime_cases(name):
        assert len(rows) <= 3000 and len(origins) <= 1 << 20
        found = bvh_cases.audit_cull(rows, origins, dirs)
        print(f"{name} / {label}: {found}")
        for key in ("rays", "answered", "excluded", "culled"):
            total[key] += found[key]
        total["slack"] = min(total["slack"], found["slack"])
        total["cases"].append((label, found))
    return total


@pytest.mark.parametrize("name", list(bvh_cases.REGIMES))
def test_no_box_on_the_way_to_the_answer_is_culled(name):
    total = audit(name)
    assert total["rays"] >= 100000
    # so that the audit cannot pass by looking at nothing: a quarter of the rays at least have a tree sphere as their answer, and
    # none is left out because the gates would hand it to the linear scan (no regime here is built for that)
    assert total["answered"] >= 0.25 * total["rays"], f"{name}: only {total['answered']} of {total['rays']} rays have a tree sphere as their answer"
    assert total["excluded"] == 0
    culled = [(label, found["first"]) for label, found in total["cases"] if found["culled"]]
    assert not culled, f"{name}: a box between the root and the answer's leaf is culled: {culled}"
    print(f"{name}: least slack {total['slack']:.4f} pad")


@pytest.mark.parametrize("axis,sign", [(0, 1.0), (1, 1.0), (2, 1.0), (0, -1.0), (1, -1.0), (2, -1.0)])
def test_the_builder_at_its_depth_limit(axis, sign):
    assert header_constant("bvh_max_depth") == STACK_DEPTH
    scene = sphere_scene(bvh_cases.cluster_chain(axis, sign))
    t = build_twice(scene)
    print(f"cluster chain, axis {axis}, sign {sign:+.0f}: depth {t['depth']}, {len(t['nodes'])} nodes, always list {list(t['always'])}")
    assert t["depth"] == STACK_DEPTH  # not <=: the scene exists to hit the limit
    assert len(t["order"]) == 333 and len(t["always"]) == 0
    if (axis, sign) == (0, 1.0):
        assert len(t["nodes"]) == 112
    check_tree(scene, t)


def test_the_always_list_takes_the_lowest_indices_of_identical_large_spheres():
    rows, large = bvh_cases.always_cap_identical()
    scene = sphere_scene(rows)
    t = build_twice(scene)
    assert 8 + len(rows) // 256 == 8
    assert t["always"].tolist() == large[:8]
    assert sorted(t["order"].tolist()) == sorted(set(range(len(rows))) - set(large[:8])) and set(large[8:]) <= set(t["order"].tolist())
    check_tree(scene, t)


def test_the_always_list_takes_the_largest_first():
    rows, large, radii = bvh_cases.always_cap_distinct()
    scene = sphere_scene(rows)
    t = build_twice(scene)
    largest = sorted(sorted(large, key=lambda i: -radii[large.index(i)])[:8])
    assert t["always"].tolist() == largest
    assert set(large) - set(largest) <= set(t["order"].tolist())
    check_tree(scene, t)


if __name__ == "__main__":
    print("# regime | rays | tree sphere is the answer | excluded by the gates | boxes culled on the way | least slack, in pads")
    for regime in bvh_cases.REGIMES:
        import contextlib
        import io

        with contextlib.redirect_stdout(io.StringIO()):
            found = audit(regime)
        print(f"{regime} | {found['rays']} | {found['answered']} ({100 * found['answered'] / found['rays']:.1f} %) | {found['excluded']} | {found['culled']} | {found['slack']:.4f}")
        for label, case in found["cases"]:
            if len(found["cases"]) > 1:
                print(f"#   {label}: {case['rays']} rays, {case['answered']} answered, slack {case['slack']:.4f}, {case['tree']} tree spheres, depth {case['depth']}")
