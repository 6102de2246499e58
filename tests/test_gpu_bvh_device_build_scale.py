"""RT_HIP_FLAG_BVH_DEVICE_BUILD past one sort tile, on the GPU (tests/test_gpu_bvh_device_build.py stops at 5000 spheres, two
tiles): the device tree of every scene of lbvh_cases.scale_names() — fields at each edge of the sort and of the per-sphere
kernels up to 262145 spheres, and the large sort, the always list and the level queues over several tiles — is the serial
restatement's byte for byte, twice over; closest hits through such trees are the linear scan's bit for bit; frames of 20481 and
100000 spheres through the product's own path equal the linear and the host-built frames.

What each scene reaches (tiles, trips of sort_scan's loop, large spheres against the cap, the widest level) is asserted on the
CPU, from the restatement alone: tests/test_bvh_lbvh_reference.py."""
import numpy as np
import pytest

import rt_amd
from rt_amd import capi
from tests import bvh_cases, lbvh_cases
from tests.bvh_cases import MATERIALS
from tests.test_gpu_bvh_device_build import rays_at, same_frame, same_hits

pytestmark = pytest.mark.gpu

BVH = capi.RT_HIP_FLAG_BVH
DEVICE = capi.RT_HIP_FLAG_BVH | capi.RT_HIP_FLAG_BVH_DEVICE_BUILD
SM = capi.RT_HIP_FLAG_SM_MATERIALS
CHECK_TREE_UP_TO = 100000  # bvh_cases.check_tree walks the tree in Python: beyond this the bytes alone are compared


@pytest.fixture(scope="module")
def tracer():
    """A context of this module's own, closed when the module is done: scenes of 262145 spheres grow a context's tables, its
    page-locked staging copy and its hierarchy blocks to tens of megabytes, and the session's context (conftest.py), which every
    later module renders through, is to keep the sizes the rest of the suite gives it.  The cached scenes and reference trees
    go with it."""
    with rt_amd.HipRayTracer(device=0) as own:
        yield own
    lbvh_cases.scale_case.cache_clear()


# ---- the tree's bytes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", lbvh_cases.scale_names())
def test_the_device_tree_past_one_sort_tile(tracer, name):
    rows, scene, want = lbvh_cases.scale_case(name)
    tracer.upload(scene)
    got = tracer.kat_bvh_build_device()
    assert [int(c) for c in want["counts"]] == [len(got["nodes"]), len(got["order"]), len(got["always"]), got["depth"], got["root"]]
    same, where = lbvh_cases.same_bytes(got, want)
    assert same, f"{name}: the device tree's {where} differ from the serial restatement's"
    if len(rows) <= CHECK_TREE_UP_TO:
        bvh_cases.check_tree(scene, got)
    again = tracer.kat_bvh_build_device()  # (the level queues' order varies from run to run; the bytes must not)
    same, where = lbvh_cases.same_bytes(got, again)
    assert same, f"{name}: two builds differ in {where}"


# ---- closest hits ---------------------------------------------------------------------------------------------------------
def test_closest_hit_through_a_tree_of_100000(tracer):
    rng = np.random.default_rng(100000)
    rows = lbvh_cases.sized_field_rows(100000)
    rows[:, 4] = np.arange(len(rows)) % len(MATERIALS)
    extra = []
    for j in range(20):  # duplicates far apart in the index order, and nested spheres
        extra.append(rows[1 + j * 4999])
        nested = rows[2 + j * 4871].copy()
        nested[3] *= 0.5
        extra.append(nested)
    rows = np.concatenate([rows, np.asarray(extra)])
    pod = rt_amd.scene_from_arrays(rows, [(0, 1, 0, 0.5, 2)], MATERIALS)
    near_o, near_d = bvh_cases.near_rays(rows, rng, 10000, 1.0)
    subset = rng.choice(len(rows), size=2000, replace=False)
    tangent_o, tangent_d = bvh_cases.tangent_rays(rows, rng, 10000, rng.uniform(0.5, 40.0, 10000), targets=subset)
    linear = same_hits(tracer, pod, np.concatenate([near_o, tangent_o]), np.concatenate([near_d, tangent_d]), "100040 spheres")
    assert (linear[1] == 1).mean() > 0.3


def test_closest_hit_with_an_always_list_cut_inside_a_tie(tracer):
    rows, large = lbvh_cases.large_ties()
    rng = np.random.default_rng(43)
    outside_o, outside_d = rays_at(rows, large, rng, 4000)
    near_o, near_d = bvh_cases.near_rays(rows, rng, 4000, 1.0)
    dist, kind, index, _ = same_hits(tracer, lbvh_cases.scale_case("large ties 9000")[1], np.concatenate([outside_o, near_o]), np.concatenate([outside_d, near_d]), "large ties 9000")
    assert (kind[:4000] == 1).all()
    answers = np.intersect1d(index[:4000], large)
    in_list = np.isin(answers, lbvh_cases.scale_case("large ties 9000")[2]["always"])
    assert in_list.sum() >= 10 and (~in_list).sum() >= 10  # large spheres of the list and large spheres of the tree both answer


def test_closest_hit_where_every_hit_is_a_tie_between_the_list_and_the_tree(tracer):
    rows, scene, tree = lbvh_cases.scale_case("one cell 9000")
    rng = np.random.default_rng(9000)
    outside_o, outside_d = rays_at(rows, np.arange(len(rows)), rng, 4000)
    near_o, near_d = bvh_cases.near_rays(rows, rng, 4000, 1.0)
    dist, kind, index, _ = same_hits(tracer, scene, np.concatenate([outside_o, near_o]), np.concatenate([outside_d, near_d]), "one cell 9000")
    assert (kind == 1).mean() > 0.3  # (from 30 radii away and more binary32 loses a sphere of radius 0.01: not every aimed ray hits)
    assert (index[kind == 1] == 0).all()  # 9000 equal distances: the lowest index, which the always list holds


# ---- frames through the product's own path ----------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [20481, 100000])
@pytest.mark.parametrize("flags", [0, SM], ids=["mg", "sm"])
def test_frames_of_large_fields_equal_the_linear_and_the_host_built_frames(tracer, count, flags):
    width, height, spp = 64, 48, 2
    rows = lbvh_cases.sized_field_rows(count)
    rows[:, 4] = np.arange(count) % len(MATERIALS)
    camera = rt_amd.Scene.parse("").set_camera((0.0, 4.0, 3.0), (0.0, -0.35, -1.0))
    ivp = camera.describe(width, height).inverse_view_projection[:]
    pod = rt_amd.scene_from_arrays(rows, [], MATERIALS, samples_per_pixel=spp, max_bounces=7, inverse_view_projection=ivp)
    linear = tracer.render(pod, width, height, seed=count, flags=flags, want_rgb=True)
    host = tracer.render(pod, width, height, seed=count, flags=flags | BVH, want_rgb=True)
    got = tracer.render(pod, width, height, seed=count, flags=flags | DEVICE, want_rgb=True)
    assert got[2]["kernel"] == "bvh" and host[2]["kernel"] == "bvh"
    same_frame(got, linear, f"{count} spheres, device tree against the linear frame")
    same_frame(got, host, f"{count} spheres, device tree against the host tree")
    assert len(np.unique(linear[0])) > 50  # the field is in the picture
