"""No plan stands that a workgroup's LDS does not hold (rt_amd/csrc/launch_plan.cpp, launch_request::lds_limit), on the CPU.

The tile-per-wave kernels park a pixel's chunk sums in LDS behind their tables: 192 bytes per chunk of the four tiles of a workgroup
once a tile is down to four pixels.  Behind the hierarchy kernel's 24 KiB of traversal stacks that is 65 472 bytes at 3408 samples,
65 664 at 3409 and 73 728 at 4096 — more than the 64 KiB a workgroup may ask for unless the device says otherwise.  plan_launch
refuses such a plan with the sample count that does fit; render.hip hands it the limit the device reports.  Here: a grid of requests
of every kind under three limits, the exact sizes the GPU tests (tests/test_gpu_chunk_sweep.py) rely on, and the refusal's text."""
import itertools

import pytest

from rt_amd import capi
from tests import lds_plan

BVH = capi.RT_HIP_FLAG_BVH
SM = capi.RT_HIP_FLAG_SM_MATERIALS
WHOLE = capi.RT_HIP_FLAG_FORCE_WHOLE_CHUNKS
BOXES = capi.RT_HIP_FLAG_TRACE_BOXES
TREE = BOXES | capi.RT_HIP_FLAG_BOX_BVH
KIB = 1024
W, H = 13, 7

SAMPLES = [16, 17, 33, 71, 144, 250, 272, 520, 1000, 3408, 3409, 4081, 4096]
# (spheres, planes, flags): the scalar-register kernel's scene, the LDS scan's last, the scalar-load scan, a large resident scene, the fullest
# LDS table there is, the hierarchy by its flag, and a scene of the streamed kernel's size (the hierarchy for passes and boxes)
SCENES = [(4, 0, 0), (39, 0, 0), (45, 1, 0), (700, 2, 0), (0, 1024, 0), (300, 0, BVH), (1500, 0, 0)]
LIMITS = [0, 64 * KIB, 160 * KIB]  # the plan's default, the same said aloud, and all of a CDNA4 compute unit's LDS
STACKS = 24 * KIB


def grid():
    """(kind, request) for every kind x scene x sample count x destination x limit, and both tables."""
    rows = []
    for (spheres, planes, flags), spp, host, limit, table in itertools.product(SCENES, SAMPLES, (0, 1), LIMITS, (0, SM)):
        common = dict(host_frame=host, lds_limit=limit)
        rows.append(("one-shot", lds_plan.request(spheres, planes, W, H, spp, flags=flags | table, **common)))
        if not table:
            rows.append(("one-shot", lds_plan.request(spheres, planes, W, H, spp, flags=flags | WHOLE, **common)))
        # one pass of `spp` samples after a first pass of 16, and an adaptive one (a pass ends on a whole chunk, or on the frame's last sample)
        rows.append(("pass", lds_plan.request(spheres, planes, W, H, 16 + spp, flags=flags | table, pass_first=16, pass_samples=spp, **common)))
        rows.append(("adaptive", lds_plan.request(spheres, planes, W, H, 16 + spp, flags=flags | table, pass_first=16, pass_samples=spp, adaptive=1, **common)))
        for boxes, box_flags in ((5, BOXES), (256, BOXES), (300, TREE)):
            rows.append(("box", lds_plan.request(spheres, planes, W, H, spp, n_boxes=boxes, flags=flags | table | box_flags, **common)))
    return rows


@pytest.fixture(scope="module")
def planned():
    if lds_plan.executable() is None:
        pytest.skip("no g++")
    rows = grid()
    return [(kind, r, p) for (kind, r), p in zip(rows, lds_plan.plans([r for _, r in rows]))]


def test_no_plan_stands_that_the_limit_does_not_hold(planned):
    refused, seen = {}, set()
    for kind, r, p in planned:
        where = f"{kind} {r} -> {p}"
        limit = r[-1] or p["default_lds_limit"]
        assert p["default_lds_limit"] == 64 * KIB and p["max_slot_bytes"] == 48 * KIB, where
        assert p["lds_bytes"] == p["table_bytes"] + p["slot_bytes"], where
        assert p["slot_bytes"] <= p["max_slot_bytes"], where  # (up to 4096 samples: the counts beyond are refused by the sample count)
        if not p["refusal"]:
            assert p["lds_bytes"] <= limit, where
        elif kind == "box":  # the box builds are planned within 64 KiB whatever the device gives, and say which flag
            assert p["lds_bytes"] > 64 * KIB and ("RT_HIP_FLAG_TRACE_BOXES" in p["refusal"] or "RT_HIP_FLAG_BOX_BVH" in p["refusal"]), where
        else:  # no refusal without need
            assert p["lds_bytes"] > limit and f"{limit}" in p["refusal"], where
        if p["refusal"]:
            refused[kind] = refused.get(kind, 0) + 1
            # only behind the hierarchy's stacks do tables and slots outgrow 64 KiB — or, with staged boxes, behind the fullest resident table
            assert p["scan"] == -4 or (kind == "box" and r[:2] == (0, 1024)), where
        seen.add((kind, p["scan"], p["planes"], p["sm_table"], p["halves"]))
        # the bits that say which build runs: a pass, an adaptive pass and a box frame are whole-chunk builds of the two tile-per-wave scans
        assert (p["pass"], p["adaptive"]) == ((1, 0) if kind == "pass" else (1, 1) if kind == "adaptive" else (0, 0)), where
        if kind != "one-shot":
            assert p["halves"] == 0 and p["scan"] in (0, -4) and not p["big_scene"], where
        assert p["boxes"] == (kind == "box") and p["box_tree"] == (kind == "box" and bool(r[7] & capi.RT_HIP_FLAG_BOX_BVH)), where
    assert set(refused) == {"one-shot", "pass", "adaptive", "box"}, refused
    # the grid reaches every tile-per-wave scan with both tables, and sub-chunk items
    for kind in ("one-shot", "pass", "adaptive", "box"):
        assert {(0, 0), (0, 1), (-4, 0)} <= {(scan, planes) for k, scan, planes, _, _ in seen if k == kind}, kind
        assert {0, 1} == {sm for k, _, _, sm, _ in seen if k == kind}, kind
    assert any(halves for k, scan, _, _, halves in seen if k == "one-shot" and scan == -4)


def test_the_fullest_resident_table_at_4096_samples_is_exactly_a_workgroups_lds():
    for host in (0, 1):
        p = lds_plan.plan(0, 1024, W, H, 4096, host_frame=host)
        assert (p["scan"], p["table_bytes"], p["slot_bytes"], p["lds_bytes"], p["refusal"]) == (0, 16 * KIB, 48 * KIB, 64 * KIB, "")


# spp: (K, pixels_log2 auto, pixels_log2 in whole chunks, HALF under auto, LDS bytes auto, LDS bytes in whole chunks) of the hierarchy kernel, 13 x 7
HIERARCHY = {
    17: (2, 4, 5, 1, 38400, 27648),
    33: (3, 3, 4, 1, 34944, 26880),
    71: (5, 2, 3, 1, 33216, 26496),
    144: (9, 2, 2, 1, 40128, 26304),
    250: (16, 2, 2, 1, 52224, 27648),
    272: (17, 2, 2, 0, 27840, 27840),
    520: (33, 2, 2, 0, 30912, 30912),
    1000: (63, 2, 2, 0, 36672, 36672),
    3408: (213, 2, 2, 0, 65472, 65472),
    3409: (214, 2, 2, 0, 65664, 65664),
    4081: (256, 2, 2, 0, 73728, 73728),
    4096: (256, 2, 2, 0, 73728, 73728),
}


@pytest.mark.parametrize("host", [0, 1])
def test_the_hierarchy_kernels_plans_are_the_ones_the_gpu_tests_rely_on(host):
    for spp, (chunks, log2_auto, log2_whole, half, lds_auto, lds_whole) in HIERARCHY.items():
        auto = lds_plan.plan(300, 1, W, H, spp, flags=BVH, host_frame=host, lds_limit=160 * KIB)
        whole = lds_plan.plan(300, 1, W, H, spp, flags=BVH | WHOLE, host_frame=host, lds_limit=160 * KIB)
        sm = lds_plan.plan(300, 1, W, H, spp, flags=BVH | SM, host_frame=host, lds_limit=160 * KIB)
        assert (auto["scan"], auto["chunks"], auto["pixels_log2"], auto["halves"], auto["sub_chunk_items"], auto["lds_bytes"], auto["refusal"]) == (-4, chunks, log2_auto, half, half, lds_auto, ""), spp
        assert (whole["scan"], whole["chunks"], whole["pixels_log2"], whole["halves"], whole["lds_bytes"], whole["table_bytes"]) == (-4, chunks, log2_whole, 0, lds_whole, STACKS), spp
        assert {k: v for k, v in sm.items() if k != "sm_table"} == {k: v for k, v in whole.items() if k != "sm_table"} and sm["sm_table"] == 1, spp
        # tile shapes: rows as wide as the tile allows for a page-locked frame, near-square tiles in HBM
        for p in (auto, whole):
            assert p["tile_w_log2"] == (min(p["pixels_log2"], 4) if host else (p["pixels_log2"] + 1) // 2), (spp, p)
        assert (auto["grid_x"], auto["grid_y"]) == ((auto["tiles_x"] + 3) // 4, auto["tiles_y"])
    shapes = {(p["pixels_log2"], p["tile_w_log2"]) for spp in (17, 33, 71) for p in [lds_plan.plan(300, 1, W, H, spp, flags=BVH | WHOLE, host_frame=host)]}
    assert shapes == ({(5, 4), (4, 4), (3, 3)} if host else {(5, 3), (4, 2), (3, 2)})
    small = {(p["pixels_log2"], p["tile_w_log2"]) for spp in (17, 33, 71) for p in [lds_plan.plan(300, 1, W, H, spp, flags=BVH, host_frame=host)]}
    assert small == ({(4, 4), (3, 3), (2, 2)} if host else {(4, 2), (3, 2), (2, 1)})  # 16 x 1, 8 x 1, 4 x 1 | 4 x 4, 4 x 2, 2 x 2


@pytest.mark.parametrize("limit", [0, 64 * KIB])
def test_the_refusal_says_how_many_samples_fit(limit):
    said = limit or 64 * KIB
    fits = lds_plan.plan(300, 1, W, H, 3408, flags=BVH, lds_limit=limit)
    assert fits["refusal"] == "" and fits["lds_bytes"] == 65472
    for flags in (BVH, BVH | SM, BVH | WHOLE):
        for spp in (3409, 4081, 4096):
            p = lds_plan.plan(300, 1, W, H, spp, flags=flags, lds_limit=limit)
            assert p["refusal"] == (f"{spp} samples per pixel need {p['lds_bytes']} bytes of LDS ({STACKS} of tables, {p['slot_bytes']} of chunk sums) and a workgroup of this device has {said}: "
                                    "at most 3408 samples fit"), p["refusal"]
    # a pass and an adaptive pass, by the flag and by the scene's size: the PASS's samples count, whatever the frame's
    for spheres, flags in ((300, BVH), (1500, 0)):
        for adaptive in (0, 1):
            ok = lds_plan.plan(spheres, 0, W, H, 9000, flags=flags, pass_first=32, pass_samples=3408, adaptive=adaptive, lds_limit=limit)
            assert ok["refusal"] == "" and ok["scan"] == -4 and ok["first_chunk"] == 2
            p = lds_plan.plan(spheres, 0, W, H, 9000, flags=flags, pass_first=32, pass_samples=3424, adaptive=adaptive, lds_limit=limit)
            assert p["refusal"] == f"a pass of 3424 samples needs 65664 bytes of LDS ({STACKS} of tables, 41088 of chunk sums) and a workgroup of this device has {said}: at most 3408 samples fit", p["refusal"]
    # what the device admits stands: with all of a compute unit's LDS the largest one-shot frame and the largest pass are planned
    for spp in (3409, 4096):
        assert lds_plan.plan(300, 1, W, H, spp, flags=BVH, lds_limit=160 * KIB)["refusal"] == ""
    assert lds_plan.plan(1500, 0, W, H, 9000, pass_first=32, pass_samples=4096, lds_limit=160 * KIB)["refusal"] == ""
    # ... and a limit below the default is kept too
    tight = lds_plan.plan(300, 1, W, H, 2000, flags=BVH, lds_limit=32 * KIB)
    assert tight["lds_bytes"] == STACKS + 125 * 192 and "at most 672 samples fit" in tight["refusal"]
    assert lds_plan.plan(300, 1, W, H, 672, flags=BVH, lds_limit=32 * KIB)["refusal"] == ""


def test_the_box_builds_limits_are_where_the_gpu_tests_look_for_them():
    """The staged-box build of the hierarchy kernel: stacks + 32 bytes per box + 192 per chunk within 64 KiB; the tree build stages nothing."""
    for boxes, flags, table in ((7, BVH | BOXES, STACKS + 7 * 32), (300, TREE, STACKS), (2, BOXES, STACKS + 2 * 32)):
        spheres = 1400 if flags == BOXES else 200
        last = (64 * KIB - table) // 192 * 16
        p = lds_plan.plan(spheres, 1, W, H, last, n_boxes=boxes, flags=flags, lds_limit=160 * KIB)
        assert p["refusal"] == "" and p["table_bytes"] == table and p["scan"] == -4 and p["lds_bytes"] <= 64 * KIB < p["lds_bytes"] + 192
        p = lds_plan.plan(spheres, 1, W, H, last + 1, n_boxes=boxes, flags=flags, lds_limit=160 * KIB)
        assert ("RT_HIP_FLAG_BOX_BVH" if flags == TREE else "RT_HIP_FLAG_TRACE_BOXES") in p["refusal"]
    # the resident kernel's box builds hold 4096 samples with every box count
    assert lds_plan.plan(45, 1, W, H, 4096, n_boxes=256, flags=BOXES)["refusal"] == ""
