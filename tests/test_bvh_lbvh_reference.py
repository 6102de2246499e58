"""The device builder of the sphere hierarchy (RT_HIP_FLAG_BVH_DEVICE_BUILD, rt_amd/csrc/bvh_build.hip) on the CPU: its serial
restatement over the same per-element header (tests/native/lbvh_reference.cpp + rt_amd/csrc/bvh_build.hpp, g++ alone).  The
traversal returns the linear scan's answer for any tree with conservative boxes, a ball around every tree sphere, leaves of at
most four and a depth of at most 24: those are checked here, tree by tree; tests/test_gpu_bvh_device_build.py then holds the
device tree to these bytes.

The depth cap: under this builder bvh_cases.cluster_chain needs no cap — 1024 Morton cells an axis put every cluster from 16^-3
inwards into one cell, where the scene indices' bits halve them (the model's depth is asserted below, and it is below 24).  The
scene that engages the cap here is lbvh_cases.morton_staircase, one cluster per Morton bit."""
import re

import numpy as np
import pytest

import rt_amd
from rt_amd.renderer import bvh_build
from tests import bvh_cases, lbvh_cases
from tests.bvh_cases import LEAF, STACK_DEPTH, geometry_of, leaf_range, sphere_scene

pytestmark = pytest.mark.skipif(lbvh_cases.reference_binary() is None, reason="no g++")

F32 = np.float32


def at_or_below(v):
    f = v.astype(F32)
    return np.where(f.astype(np.float64) > v, np.nextafter(f, F32(-np.inf)), f)


def at_or_above(v):
    f = v.astype(F32)
    return np.where(f.astype(np.float64) < v, np.nextafter(f, F32(np.inf)), f)


def check_boxes_are_tight(scene, t):
    """Each child box against the float64 union of its spheres' boxes: not inside it, and at most one binary32 step outside."""
    if len(t["order"]) == 0:
        return 0
    g = geometry_of(scene)[t["order"]].astype(np.float64)
    half = np.sqrt(g[:, 3])
    lo, hi = g[:, :3] - half[:, None], g[:, :3] + half[:, None]
    nodes = t["nodes"]
    links = nodes[:, [3, 7]].copy().view(np.uint32)
    checked = 0
    todo = [int(t["root"])]
    span = {}  # node -> (first, count) of the leaf slots below it

    def slots(link):
        if link & LEAF:
            return leaf_range(link)
        if link not in span:
            a, b = slots(int(links[link, 0])), slots(int(links[link, 1]))
            assert a[0] + a[1] == b[0]  # the halves of a sorted range
            span[link] = (a[0], a[1] + b[1])
        return span[link]

    while todo:
        link = todo.pop()
        if link & LEAF:
            continue
        for which in (0, 1):
            child = int(links[link, which])
            first, count = slots(child)
            want_lo, want_hi = at_or_below(lo[first : first + count].min(axis=0)), at_or_above(hi[first : first + count].max(axis=0))
            got_lo, got_hi = nodes[link, which * 8 : which * 8 + 3], nodes[link, which * 8 + 4 : which * 8 + 7]
            assert (got_lo <= want_lo).all() and (got_lo >= np.nextafter(want_lo, F32(-np.inf))).all(), f"node {link} child {which}: min {got_lo}, the union's {want_lo}"
            assert (got_hi >= want_hi).all() and (got_hi <= np.nextafter(want_hi, F32(np.inf))).all(), f"node {link} child {which}: max {got_hi}, the union's {want_hi}"
            checked += 1
            todo.append(child)
    return checked


@pytest.mark.parametrize("name", lbvh_cases.scene_names())
def test_the_reference_tree_is_one_the_traversal_can_use(name):
    for rows in lbvh_cases.scenes_of(name):
        scene = sphere_scene(rows)
        t = lbvh_cases.reference_tree(scene)
        bvh_cases.check_tree(scene, t)
        assert t["depth"] <= STACK_DEPTH
        # the always list and the tree's members are the host builder's
        host = bvh_build(scene)
        assert np.array_equal(t["always"], host["always"])
        assert np.array_equal(np.sort(t["order"]), np.sort(host["order"]))
        # the order is the order of (Morton code, scene index), worked out again in numpy
        if len(t["order"]):
            keys = lbvh_cases.model_keys(geometry_of(scene), t["order"])
            assert np.array_equal((keys & np.uint64(0xFFFFFFFF)).astype(np.uint32), t["order"])
        inner = check_boxes_are_tight(scene, t)
        assert (inner > 0) == (len(t["order"]) > 4)
        again = lbvh_cases.reference_tree(scene)
        assert lbvh_cases.same_bytes(t, again)[0]


# ---- past one sort tile -----------------------------------------------------------------------------------------------------
BOX_WALK_UP_TO = 100000


def test_the_sizes_sit_on_the_edges_of_the_builders_constants():
    """lbvh_cases.SIZED_FIELDS is chosen for threads = 256, sort_rounds = 16 and scan_threads = 1024: a retuned sort must not
    move the edges away from the sizes without this failing."""
    text = (lbvh_cases.ROOT / "rt_amd" / "csrc" / "bvh_build.hip").read_text()

    def constant(name):
        found = re.findall(rf"constexpr uint32_t {name} = (\d+);", text)
        assert len(found) == 1, name
        return int(found[0])

    assert (constant("threads"), constant("sort_rounds"), constant("scan_threads")) == (256, 16, 1024)
    assert "constexpr uint32_t sort_tile = threads * sort_rounds;" in text
    assert (lbvh_cases.THREADS, lbvh_cases.SORT_ROUNDS, lbvh_cases.SCAN_THREADS, lbvh_cases.SORT_TILE) == (256, 16, 1024, 4096)
    assert "bins[256]" in text and "& 255u" in text and lbvh_cases.DIGITS == 256  # eight bits a pass


@pytest.mark.parametrize("name", lbvh_cases.scale_names())
def test_the_reference_tree_past_one_sort_tile(name):
    """test_the_reference_tree_is_one_the_traversal_can_use on lbvh_cases.scale_names().  check_boxes_are_tight walks the tree
    in Python, seven seconds at 262145 spheres: it runs up to 100000 spheres only.  check_tree, the host builder's always list
    and members, and model_keys hold at every size."""
    rows, scene, t = lbvh_cases.scale_case(name)
    bvh_cases.check_tree(scene, t)
    assert t["depth"] <= STACK_DEPTH
    host = bvh_build(scene)
    assert np.array_equal(t["always"], host["always"])
    assert np.array_equal(np.sort(t["order"]), np.sort(host["order"]))
    if len(t["order"]):
        keys = lbvh_cases.model_keys(geometry_of(scene), t["order"])
        assert np.array_equal((keys & np.uint64(0xFFFFFFFF)).astype(np.uint32), t["order"])
    if len(rows) <= BOX_WALK_UP_TO:
        inner = check_boxes_are_tight(scene, t)
        assert (inner > 0) == (len(t["order"]) > 4)
    again = lbvh_cases.reference_tree(scene)
    assert lbvh_cases.same_bytes(t, again)[0]


def r2_bits(scene):
    return geometry_of(scene)[:, 3].view(np.uint32)


def cut_of_the_always_list(scene, t):
    """The r^2 bits at the cap's cut, and the large spheres that have them (ascending): inside the list, outside it."""
    tame, large = lbvh_cases.large_spheres(geometry_of(scene))
    bits = r2_bits(scene)
    taken = t["always"][tame[t["always"]]]
    at_cut = bits[taken].min()
    group = np.nonzero(large & (bits == at_cut))[0]
    inside = np.isin(group, taken)
    return group[inside], group[~inside]


@pytest.mark.parametrize("name", lbvh_cases.scale_names())
def test_each_scene_past_one_sort_tile_reaches_what_it_is_named_for(name):
    """From n, the (c, r^2) table and the restatement's tree alone: the sort tiles, sort_scan's trips, the large spheres
    against the cap, where the always list comes from, and the widest level against a block of build_level."""
    rows, scene, t = lbvh_cases.scale_case(name)
    n = len(rows)
    reach = lbvh_cases.reach(scene, t)
    print(name, reach)
    assert reach["tiles"] == -(-n // 4096) and reach["scan trips"] == -(-256 * reach["tiles"] // 1024) and reach["cap"] == 8 + n // 256
    if name.startswith("sized field "):
        assert (reach["tiles"], reach["scan trips"]) == lbvh_cases.SIZED_FIELDS[n]
        assert reach["n_large"] == 1 and t["always"].tolist() == [0] and not reach["large sort runs"]  # the ground sphere
        if n >= 4095:
            assert reach["widest level"] > 256  # build_level and build_refit hand out slots from more than one block
        if n >= 16384:
            assert reach["widest level"] > 4 * 256 and reach["level blocks at the bound"] > 4
        return
    assert reach["tiles"] >= 2
    if name == "one cell 9000":
        assert (reach["tiles"], reach["n_large"], reach["cap"]) == (3, 9000, 43) and reach["large sort runs"]
        assert t["always"].tolist() == list(range(43)) and t["order"].tolist() == list(range(43, 9000))
        keys = lbvh_cases.model_keys(geometry_of(scene), t["order"])
        assert len(np.unique(keys >> np.uint64(32))) == 1  # one Morton cell: the index alone decides
    elif name == "two cells 9001":
        assert (reach["tiles"], reach["n_large"], reach["always"]) == (3, 0, 0)
        assert t["order"].tolist() == list(range(0, 9001, 2)) + list(range(1, 9001, 2))
    elif name == "large ties 9000":
        large = lbvh_cases.large_ties()[1]
        assert (reach["tiles"], reach["n_large"], reach["cap"], reach["always"]) == (3, 80, 43, 43) and reach["large sort runs"]
        assert np.array_equal(np.nonzero(lbvh_cases.large_spheres(geometry_of(scene))[1])[0], large)
        assert sorted(set((large // 4096).tolist())) == [0, 1, 2] and len(reach["taken tiles"]) >= 2
        assert np.unique(r2_bits(scene)[large], return_counts=True)[1].tolist() == [4] * 20
        inside, outside = cut_of_the_always_list(scene, t)
        assert len(inside) == 3 and len(outside) == 1 and inside.max() < outside.min()  # the cut goes to the lowest indices
    elif name in ("large at the cap", "large one above the cap"):
        above = name == "large one above the cap"
        assert (reach["tiles"], reach["cap"], reach["n_large"], reach["always"]) == (2, 27, 28 if above else 27, 27)
        assert reach["large sort runs"] == above  # 28 is the fewest that run it
        assert reach["taken tiles"] == [0, 1]
    elif name == "large over sixty binades":
        assert (reach["tiles"], reach["n_large"], reach["cap"], reach["always"]) == (2, 6000, 31, 31) and reach["large sort runs"]
        bits = r2_bits(scene)
        assert bits.min() >= np.float32(1e-38).view(np.uint32) and bits.max() <= np.float32(2.0**80).view(np.uint32)
        for shift in (0, 8, 16, 24):  # every pass of the large sort has keys to tell apart
            assert len(np.unique((~bits >> np.uint32(shift)) & np.uint32(255))) >= 64
        assert (np.unique(bits, return_counts=True)[1] == 2).sum() >= 2  # two pairs of equal r^2 ...
        inside, outside = cut_of_the_always_list(scene, t)
        assert len(inside) == 1 and len(outside) == 1 and inside[0] < outside[0]  # ... one of them at the cut
        largest = np.lexsort((np.arange(n), ~bits))[:31]  # by (larger r^2, lower index)
        assert np.array_equal(t["always"], np.sort(largest))
    elif name == "mostly non-finite 9000":
        assert (reach["tiles"], reach["n_large"], reach["always"], len(t["order"])) == (3, 1, 8991, 9)
        assert reach["always tiles"] == [0, 1, 2] and not reach["large sort runs"]
    else:
        raise AssertionError(f"{name} states nothing about itself")


def test_check_tree_accepts_the_host_builders_trees():
    """The checker itself, on trees it is known to hold for."""
    for name in ("field 300", "always cap distinct", "chain x"):
        for rows in lbvh_cases.scenes_of(name):
            scene = sphere_scene(rows)
            bvh_cases.check_tree(scene, bvh_build(scene))


def test_small_scenes_have_the_expected_shape():
    for count, nodes in ((2, 0), (4, 0), (5, 4), (8, 7), (9, 8)):
        rows = np.zeros((count, 5))
        rows[:, 0] = np.arange(count)  # no large sphere: every one is in the tree
        rows[:, 3] = 0.1
        t = lbvh_cases.reference_tree(sphere_scene(rows))
        assert len(t["order"]) == count and len(t["always"]) == 0 and len(t["nodes"]) == nodes
        assert bool(t["root"] & LEAF) == (count <= 4)
    everything_out = lbvh_cases.reference_tree(sphere_scene(lbvh_cases.non_finite()))
    assert len(everything_out["order"]) == 0 and everything_out["always"].tolist() == list(range(12)) and everything_out["depth"] == 0
    identical = lbvh_cases.reference_tree(sphere_scene(lbvh_cases.scenes_of("64 identical")[0]))
    assert identical["always"].tolist() == list(range(8)) and identical["order"].tolist() == list(range(8, 64))  # one Morton cell: the index decides


def test_the_always_lists_caps():
    rows, large = bvh_cases.always_cap_identical()
    t = lbvh_cases.reference_tree(sphere_scene(rows))
    assert t["always"].tolist() == large[:8] and set(large[8:]) <= set(t["order"].tolist())
    rows, large, radii = bvh_cases.always_cap_distinct()
    t = lbvh_cases.reference_tree(sphere_scene(rows))
    assert t["always"].tolist() == sorted(large[k] for k in np.argsort(radii)[-8:])


def test_the_depth_cap_engages():
    """Without the cap the staircase's tree is deeper than the traversal's stack; the reference's is exactly as deep as it."""
    scene = sphere_scene(lbvh_cases.morton_staircase())
    t = lbvh_cases.reference_tree(scene)
    uncapped = lbvh_cases.uncapped_depth(lbvh_cases.model_keys(geometry_of(scene), t["order"]))
    print(f"morton staircase: uncapped depth {uncapped}, reference depth {t['depth']}")
    assert uncapped > STACK_DEPTH
    assert t["depth"] == STACK_DEPTH


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_the_cluster_chain_stays_within_the_stack(axis):
    """bvh_cases.cluster_chain engages the HOST builder's cap (sixteen bins peel off one cluster a level).  This builder's
    30-bit code cannot tell its inner clusters apart, so its uncapped tree is shallow already: the model says how shallow, and
    the reference must agree with the model (no cap, no difference)."""
    scene = sphere_scene(bvh_cases.cluster_chain(axis, 1.0))
    t = lbvh_cases.reference_tree(scene)
    uncapped = lbvh_cases.uncapped_depth(lbvh_cases.model_keys(geometry_of(scene), t["order"]))
    print(f"cluster chain on axis {axis}: uncapped depth {uncapped}, reference depth {t['depth']}")
    assert t["depth"] <= STACK_DEPTH
    assert uncapped <= STACK_DEPTH and t["depth"] == uncapped


@pytest.mark.parametrize("name", ["scale sweep", "duplicates"])
def test_no_box_on_the_way_to_the_answer_is_culled(name, monkeypatch):
    """bvh_cases.audit_cull on the reference's trees: the cull bound holds whatever the tree's shape."""
    monkeypatch.setattr(rt_amd.renderer, "bvh_build", lbvh_cases.reference_tree)
    total = {"rays": 0, "answered": 0, "excluded": 0}
    for label, rows, origins, dirs in lbvh_cases.regime(name):
        found = bvh_cases.audit_cull(rows, origins, dirs)
        assert found["culled"] == 0, f"{name} / {label}: a box between the root and the answer's leaf is culled: {found.get('first')}"
        assert found["depth"] <= STACK_DEPTH and found["tree"] == len(rows)
        for key in total:
            total[key] += found[key]
    assert total["answered"] >= 0.25 * total["rays"] and total["excluded"] == 0
