"""The box hierarchy of RT_HIP_FLAG_BOX_BVH, as built on the host (rt_hip_kat_box_bvh_build: no GPU; rt_amd/csrc/box_bvh.cpp).

What the traversal's "same answer as the linear scan" rests on (rt_amd/csrc/box_bvh_scan.hpp), checked on the builder's output: every
box is in exactly one leaf slot or in the always list, every child box is the EXACT union of the extents below it (the cull has no
pad to hide a rounding in), the depth stays within the traversal stack, the leaf table holds bit copies of the uploaded pairs, boxes
with a non-finite corner stay out of the tree, and two builds are the same bytes.  The GPU side is tests/test_gpu_box_bvh.py."""
import subprocess

import numpy as np
import pytest

from rt_amd import capi
from rt_amd.renderer import box_bvh_build
from tests import box_bvh_cases as cases
from tests.box_bvh_cases import box_scene, build_twice, check_box_tree
from tests.bvh_cases import LEAF, STACK_DEPTH
from tests.conftest import ROOT


def field(count, seed=1):
    return cases.random_boxes(np.random.default_rng(seed), count, spread=6.0)


@pytest.mark.parametrize("count", [0, 1, 4, 5, 257, 5000])
def test_counts(count):
    scene = box_scene(field(count))
    t = build_twice(scene)
    check_box_tree(scene, t)
    assert len(t["order"]) + len(t["always"]) == count
    if count == 0:
        assert len(t["nodes"]) == 0 and len(t["order"]) == 0
    if count in (1, 4):
        assert len(t["nodes"]) == 0 and t["depth"] == 0 and t["root"] & LEAF, "the root is a leaf"
    if count == 5:
        assert len(t["order"]) == 5 and len(t["nodes"]) == 1 and t["depth"] == 1 and t["root"] == 0, "one inner node"
    if count >= 257:
        assert len(t["always"]) <= 8 + count // 256 and t["depth"] <= STACK_DEPTH


def test_64_identical_boxes():
    scene = box_scene([(1, 2, 3, 0.5, 0.25, 0.125, i % 4) for i in range(64)])
    t = build_twice(scene)
    check_box_tree(scene, t)
    assert len(t["order"]) == 64 and len(t["always"]) == 0  # (no extent among the centres: nothing is "large")
    assert t["depth"] == 4  # median splits by index: 64 -> 16 leaves of four


@pytest.mark.parametrize("axis,sign", [(0, 1.0), (1, -1.0), (2, 1.0)])
def test_the_builder_at_its_depth_limit(axis, sign):
    scene = box_scene(cases.chain_boxes(axis, sign))
    t = build_twice(scene)
    print(f"chain, axis {axis}, sign {sign:+.0f}: depth {t['depth']}, {len(t['nodes'])} nodes, always list {list(t['always'])}")
    assert t["depth"] == STACK_DEPTH  # not <=: the scene exists to hit the limit
    assert len(t["order"]) == 333 and len(t["always"]) == 0
    check_box_tree(scene, t)


def test_boxes_with_lo_above_hi():
    """Negative extents: the uploaded pair has lo > hi on those axes, the tree's extent is the swapped box's, the leaf slot the pair's."""
    rows = field(40, seed=2)
    rows[::3, 3] *= -1
    rows[1::4, 4:6] *= -1
    scene = box_scene(rows)
    bounds = cases.bounds_of(scene)
    assert (bounds[:, 0] > bounds[:, 4]).sum() >= 10
    t = build_twice(scene)
    check_box_tree(scene, t)
    assert len(t["always"]) == 0


def test_boxes_with_nan_and_infinite_corners():
    rows = field(30, seed=3)
    rows[4, 0] = np.nan
    rows[9, 4] = np.inf  # (centre -/+ inf: both corners infinite on y)
    rows[15, 2] = -np.inf
    rows[21, 5] = np.nan
    rows[22, 3] = 3e38  # finite columns, an infinite corner: centre + extent overflows for a centre of 3e38
    rows[22, 0] = 3e38
    scene = box_scene(rows)
    t = build_twice(scene)
    check_box_tree(scene, t)
    assert {4, 9, 15, 21, 22} <= set(t["always"].tolist())


def test_a_large_slab_stays_out_of_the_tree():
    rows = np.concatenate([[(0, -0.5, 0, 100, 0.5, 100, 0)], field(300, seed=4)])
    scene = box_scene(rows)
    t = build_twice(scene)
    check_box_tree(scene, t)
    assert 0 in set(t["always"].tolist())


def test_leaf_slots_carry_the_material_bits():
    scene = box_scene([(i, 0, 0, 0.1, 0.1, 0.1, i % 4) for i in range(9)])
    t = box_bvh_build(scene)
    assert t["corners"][:, 3].copy().view(np.uint32).tolist() == [int(i) % 4 for i in t["order"]]
    assert (t["corners"][:, 7] == 0).all()


def test_flag_constant_matches_the_header(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text('#include "rt_hip.h"\n#include <stdio.h>\nint main(void) { printf("%u %u %u\\n", (unsigned)RT_HIP_FLAG_BOX_BVH, (unsigned)RT_HIP_FLAG_TRACE_BOXES, (unsigned)RT_HIP_ABI_VERSION); return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.run(["cc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    flag, boxes, abi = (int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert (flag, boxes, abi) == (capi.RT_HIP_FLAG_BOX_BVH, capi.RT_HIP_FLAG_TRACE_BOXES, capi.RT_HIP_ABI_VERSION)
    assert flag == 1 << 14 and abi == 6
