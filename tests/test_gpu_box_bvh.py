"""RT_HIP_FLAG_BOX_BVH on the GPU: every frame is compared bit for bit — packed pixels, float mean, segments — with the
CPU restatement of the box contract (tests/native/box_reference.cpp, which takes any number of boxes), every closest hit with its
closest_hit, and the kernel that ran is the hierarchy kernel.  Tolerance 0 everywhere.  Both the mg and the sm table wherever a
material tells them apart."""
import subprocess

import numpy as np
import pytest

import rt_amd
from rt_amd import capi
from tests import box_bvh_cases as cases
from tests import box_reference as box_ref
from tests.conftest import GOLDEN, ROOT, unpack
from tests.test_gpu_boxes import check_frame

pytestmark = pytest.mark.gpu

BOXES = capi.RT_HIP_FLAG_TRACE_BOXES
TREE = BOXES | capi.RT_HIP_FLAG_BOX_BVH
SM = capi.RT_HIP_FLAG_SM_MATERIALS
UNSUPPORTED = 5
PLANE = [(0, 1, 0, 0, 0)]


def check_hits(tracer, pod, origins, directions, expect_boxes=1):
    tracer.upload(pod)
    got = tracer.kat_closest_hit(origins, directions, box_bvh=True)
    want = box_ref.closest_hit(pod, origins, directions)
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), f"{(got[1] != want[1]).sum()} kinds, {(got[2] != want[2]).sum()} indices differ"
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))
    assert np.array_equal(got[3].view(np.uint32), want[3].view(np.uint32))
    assert (want[1] == box_ref.KIND_BOX).sum() >= expect_boxes
    return want


@pytest.mark.parametrize("count", [1, 4, 5, 257])
def test_leaf_and_node_counts(tracer, count):
    """1 and 4 boxes: the root is a leaf; 5: one inner node; 257: the first count the linear build refuses."""
    boxes = cases.grid_boxes(count, pitch=0.25, half=0.1, z0=1.5)
    pod = cases.box_scene(boxes, spheres=[(0, 0.6, 0, 0.5, 1)], planes=PLANE, spp=16)
    tree = rt_amd.renderer.box_bvh_build(pod)
    assert len(tree["nodes"]) == {1: 0, 4: 0, 5: 1}.get(count, len(tree["nodes"])) and len(tree["order"]) == count
    for table in (0, SM):
        check_frame(tracer, pod, 64, 36, 20 + count, TREE | table, "bvh")
    if count == 257:
        canvas = np.full((36, 64), 0xDEADBEEF, dtype=np.uint32)
        with pytest.raises(rt_amd.RtHipError) as refused:
            tracer.render(pod, 64, 36, seed=1, flags=BOXES, out=canvas)
        assert refused.value.status == UNSUPPORTED and "257 boxes" in str(refused.value) and (canvas == 0xDEADBEEF).all()


def test_a_mixed_scene_both_trees_one_stack(tracer):
    """About 2 000 boxes with 1 400 spheres and a plane, 32x18x16."""
    from tests.test_gpu_boxes import grid_spheres

    rng = np.random.default_rng(1)
    boxes = cases.random_boxes(rng, 2000, spread=3.0, e_lo=0.02, e_hi=0.15)
    boxes[:, 1] = np.abs(boxes[:, 1]) * 0.5 + 0.1
    pod = box_ref.scene_pod(cases.camera(32, 18), spheres=grid_spheres(1400, radius=0.05, pitch=0.12), planes=PLANE, boxes=[tuple(b) for b in boxes], spp=16)
    for table in (0, SM):
        check_frame(tracer, pod, 32, 18, 2, TREE | table, "bvh")
    origins, directions = cases.rays_at(boxes, rng, 4000)
    check_hits(tracer, pod, origins, directions, 1500)


def test_boxes_only(tracer):
    """No sphere, no plane: the sphere tree is empty."""
    pod = cases.box_scene(cases.grid_boxes(40, pitch=0.4, half=0.15, z0=1.0), spp=20)
    for table in (0, SM):
        check_frame(tracer, pod, 64, 36, 3, TREE | table, "bvh")


def test_every_box_in_the_always_list_and_an_empty_tree(tracer):
    """Boxes with an infinite corner (they still hit: half spaces and slabs) next to a NaN box (never hit): the tree is empty."""
    inf = float("inf")
    boxes = [(0, -inf, 0, 1, inf, 1, 1), (2, 0.5, 0, 0.5, 0.5, inf, 2), (-2, 0.5, 0.5, 0.4, float("nan"), 0.4, 3), (-1.5, 0.4, 1, 0.3, 0.4, 0.3, 0)]
    boxes[3] = (-1.5, 0.4, -inf, 0.3, 0.4, 0.3, 0)
    pod = cases.box_scene(boxes, spheres=[(0.5, 0.5, 1.5, 0.4, 2)], spp=20)
    tree = rt_amd.renderer.box_bvh_build(pod)
    assert len(tree["order"]) == 0 and tree["always"].tolist() == [0, 1, 2, 3]
    for table in (0, SM):
        check_frame(tracer, pod, 64, 36, 4, TREE | table, "bvh")


def test_ties(tracer):
    """64 identical boxes: index 0 wins.  A box face coplanar with a plane and tangent to a sphere: the box wins."""
    same = [(0, 0.8, 0, 0.7, 0.8, 0.7, i % 4) for i in range(64)]
    pod = cases.box_scene(same, planes=PLANE, spp=20)
    want = check_hits(tracer, pod, [(0, 0.8, 3), (0.2, 5, 0.1)], [(0.01, 0.02, -1), (0.001, -1, 0.002)], 2)
    assert want[2].tolist() == [0, 0]
    for table in (0, SM):
        check_frame(tracer, pod, 64, 36, 5, TREE | table, "bvh")
    many = cases.grid_boxes(300, pitch=0.3, half=0.1, z0=-2.0)
    pod = box_ref.scene_pod(cases.camera(), box_ref.KAT_SPHERES, box_ref.KAT_PLANES, list(box_ref.KAT_BOXES) + many, spp=16)
    # box 2's top face, plane 0 and sphere 0 all at t = 2 from (10, 5, 0) straight down (tests/box_reference.py); components of finite reciprocal
    want = check_hits(tracer, pod, [(10, 5, 0), (10, 5, 0)], [(0, -1, 0), (2.0**-60, -1, -(2.0**-60))], 2)
    assert want[1].tolist() == [3, 3] and want[2].tolist() == [2, 2] and want[0].tolist() == [2.0, 2.0]


def test_origins_inside_boxes(tracer):
    """The camera inside nested boxes: exit distances and tmax are accepted.  A glass box under the sm table: rays start on faces."""
    nested = [(0, 1, 3, 0.5 * (k + 1), 0.4 * (k + 1), 0.5 * (k + 1), k % 4) for k in range(6)]
    pod = cases.box_scene(nested + cases.grid_boxes(280, pitch=0.3, half=0.1, z0=0.5), spheres=[(0, 1, 2.2, 0.2, 1)], spp=16)
    t, kind, index, normal = box_ref.closest_hit(pod, [(0, 1, 3)], [(0.001, 1, 0.002)])
    assert kind[0] == 3 and index[0] == 0 and abs(float(t[0]) - 0.4) < 1e-6  # the innermost shell's exit face (tmax)
    for table in (0, SM):
        check_frame(tracer, pod, 64, 36, 6, TREE | table, "bvh")
    glass = [(0, 0.7, 0.5, 0.8, 0.7, 0.5, 2)] + cases.grid_boxes(260, pitch=0.35, half=0.12, z0=-1.0)
    pod = cases.box_scene(glass, planes=PLANE, spp=16)
    check_frame(tracer, pod, 64, 36, 7, TREE | SM, "bvh")
    _, _, plain = tracer.render(pod, 64, 36, seed=7, flags=TREE)
    _, _, refracting = tracer.render(pod, 64, 36, seed=7, flags=TREE | SM)
    assert plain["segments"] != refracting["segments"]  # (the table is told apart)


def test_deep_tree(tracer):
    """The depth-24 chain in a frame, and a ray that fills the lane's stack as far as a straight ray can.  From beyond the innermost
    cluster outward along the chain the inner child is the nearer one at every level and the outer one waits: the model of the
    visiting order (box_bvh_cases.model_stack_depth) counts 23 of the 24 words — the last cut of the deepest path lies inside a
    cluster, whose nearer half is a leaf that is hit first and whose hit culls the other.  (The word index 23 is written by no ray
    this file could find; `depth >= bvh_max_depth` in bvh_boxes guards it.)"""
    rows = cases.chain_boxes(0, 1.0)
    rows[:, 6] = np.arange(len(rows)) % 4
    pod = box_ref.scene_pod(cases.camera_at((1.04, 0.0, 0.02), (0, 0, -1)), boxes=[tuple(r) for r in rows], planes=[(0, 1, 0, 1, 0)], spp=16)
    tree = rt_amd.renderer.box_bvh_build(pod)
    assert tree["depth"] == cases.STACK_DEPTH
    for table in (0, SM):
        check_frame(tracer, pod, 64, 36, 8, TREE | table, "bvh")
    origin, direction = (-(2.0**-120), 0.0, 0.0), (1.0, 2.0**-126, -(2.0**-126))
    assert cases.model_stack_depth(tree, cases.bounds_of(pod), origin, direction) == cases.STACK_DEPTH - 1
    rng = np.random.default_rng(9)
    more_o, more_d = cases.rays_at(rows, rng, 2000)
    want = check_hits(tracer, pod, np.concatenate([[origin], more_o]), np.concatenate([[direction], more_d]), 300)
    assert want[1][0] == 3


def test_degenerate_corners(tracer):
    """Boxes with lo > hi (negative extents), and a box with a NaN corner next to ordinary ones."""
    boxes = np.array(cases.grid_boxes(270, pitch=0.3, half=0.1, z0=1.0), dtype=np.float64)
    boxes[::2, 3] *= -1
    boxes[1::3, 4:6] *= -1
    boxes[7, 0] = np.nan
    pod = cases.box_scene(boxes, planes=PLANE, spp=16)
    tree = rt_amd.renderer.box_bvh_build(pod)
    assert tree["always"].tolist() == [7]
    for table in (0, SM):
        check_frame(tracer, pod, 64, 36, 9, TREE | table, "bvh")
    rng = np.random.default_rng(10)
    keep = np.delete(boxes, 7, axis=0)
    origins, directions = cases.rays_at(keep, rng, 3000)
    check_hits(tracer, pod, origins, directions, 1000)


def test_degenerate_rays(tracer):
    """+0, -0, subnormal and huge-reciprocal components; origins exactly on slab planes, the two grazing rays tests/box_reference.py
    pins among them; non-finite origins: the known-answer entry point against the restatement, with more than 256 boxes."""
    many = cases.grid_boxes(300, pitch=0.3, half=0.1, z0=-6.0)
    boxes = list(box_ref.KAT_BOXES) + many
    pod = box_ref.scene_pod(cases.camera(), box_ref.KAT_SPHERES, box_ref.KAT_PLANES, boxes, spp=16)
    origins, directions, expected = box_ref.known_answer_rays()
    want = check_hits(tracer, pod, origins, directions, 20)
    for i, row in enumerate(expected):  # (the hand-made answers still stand with the grid behind them)
        if row is not None:
            assert (int(want[1][i]), int(want[2][i])) == (row[0], row[1]) and (want[0][i] == np.float32(row[2])), (i, row)
    rng = np.random.default_rng(11)
    rows = np.array(boxes, dtype=np.float64)[[0, 2] + list(range(4, len(boxes)))]
    o, _ = cases.rays_at(rows, rng, 6000)
    d = cases.degenerate_directions(rng, 6000)
    taken = cases.gate_takes(o, d)
    assert (~taken).sum() > 1500 and taken.sum() > 500
    check_hits(tracer, pod, o, d, 300)
    # origins exactly on slab planes of grid boxes, running along the face (0 x inf in the linear scan and in the fall-back alike)
    lo, hi = rows[:, 0:3] - rows[:, 3:6], rows[:, 0:3] + rows[:, 3:6]
    pick = rng.integers(4, len(rows), 600)
    on = ((lo[pick] + hi[pick]) / 2).astype(np.float32)
    axis = rng.integers(0, 3, 600)
    on[np.arange(600), axis] = np.where(rng.integers(0, 2, 600) == 0, lo[pick, axis], hi[pick, axis]).astype(np.float32)
    along = cases.unit(rng.normal(size=(600, 3))).astype(np.float32)
    along[np.arange(600), axis] = np.where(rng.integers(0, 2, 600) == 0, 0.0, -0.0)
    check_hits(tracer, pod, on - along * np.float32(0.5), along, 50)
    bad = o[:12].copy()
    bad[np.arange(12), np.arange(12) % 3] = [np.inf, -np.inf, np.nan] * 4
    # (against the boxes alone: the plane and sphere contracts are stated for finite origins, and this file is not about them)
    alone = box_ref.scene_pod(cases.camera(), boxes=boxes, spp=16)
    check_hits(tracer, alone, bad, cases.unit(rng.normal(size=(12, 3))).astype(np.float32), 0)
    check_hits(tracer, alone, o[:2000], d[:2000], 100)


def test_a_frame_whose_lanes_fall_back_inside_ordinary_waves(tracer):
    """An orthographic frustum: every primary ray is (0, 0, -1) exactly — two zero components, the linear scan — and every scattered
    ray is ordinary; a wave holds lanes at every bounce, so both kinds sit side by side in it."""
    from oracle import binding as oracle
    from rt_amd.scene import scene_from_arrays

    matrix = np.zeros((4, 4), dtype=np.float32)
    matrix[0, 0], matrix[1, 1], matrix[1, 3], matrix[2, 2], matrix[2, 3], matrix[3, 3] = 4, 2.25, 1, -10, 3, 1
    materials = [(kind, *albedo, 1.0, roughness, reflectivity) for kind, albedo, roughness, reflectivity in box_ref.MATERIALS]
    boxes = cases.grid_boxes(300, pitch=0.45, half=0.18, z0=0.5)
    pod = scene_from_arrays(spheres=None, planes=PLANE, materials=materials, boxes=boxes, samples_per_pixel=16, max_bounces=6, inverse_view_projection=matrix)
    for x, y in [(0, 0), (32, 18), (63, 35)]:
        _, direction, form = oracle.primary_ray(pod, 64, 36, x, y, want_form=True)
        assert direction.tolist() == [0.0, 0.0, -1.0] and form == "general"
    for table in (0, SM):
        _, stats = check_frame(tracer, pod, 64, 36, 12, TREE | table, "bvh")
        assert stats["segments"] > 64 * 36 * 16 + 1000  # (scattered rays there are)


def test_agreement_with_the_linear_build(tracer):
    """<= 256 boxes with and without the flag: identical frames (and the kernel each names)."""
    pod = cases.box_scene(cases.grid_boxes(200, pitch=0.3, half=0.1, z0=1.0), spheres=[(0, 0.7, 1.5, 0.4, 2)], planes=PLANE, spp=16)
    for table in (0, SM):
        linear = tracer.render(pod, 64, 36, seed=13, flags=BOXES | table, want_rgb=True)
        tree = tracer.render(pod, 64, 36, seed=13, flags=TREE | table, want_rgb=True)
        assert np.array_equal(linear[0], tree[0]) and np.array_equal(linear[1].view(np.uint32), tree[1].view(np.uint32))
        assert linear[2]["segments"] == tree[2]["segments"] and (linear[2]["kernel"], tree[2]["kernel"]) == ("resident", "bvh")
    check_frame(tracer, pod, 64, 36, 13, TREE, "bvh")


def test_without_a_box_the_flag_changes_nothing(tracer):
    pod = rt_amd.Scene.named("basic").set_sampling(20).describe(64, 36)
    plain = tracer.render(pod, 64, 36, seed=9, want_rgb=True)
    flagged = tracer.render(pod, 64, 36, seed=9, flags=TREE, want_rgb=True)
    assert np.array_equal(plain[0], flagged[0]) and np.array_equal(plain[1].view(np.uint32), flagged[1].view(np.uint32))
    for key in ("kernel", "segments", "primary_samples", "sphere_tests", "plane_tests"):
        assert plain[2][key] == flagged[2][key], key
    assert plain[2]["kernel"] == "small"


def test_the_tree_is_cached_with_the_context(tracer):
    """Moving one box rebuilds the tree, an unchanged scene reuses it — and so does a scene whose boxes are the same."""
    boxes = cases.grid_boxes(300, pitch=0.3, half=0.1, z0=1.0)
    pod = cases.box_scene(boxes, planes=PLANE, spp=16)
    tracer.render(pod, 64, 36, seed=1, flags=TREE)
    builds = tracer.kat_box_bvh_builds()
    check_frame(tracer, pod, 64, 36, 14, TREE, "bvh")
    assert tracer.kat_box_bvh_builds() == builds
    moved = list(boxes)
    moved[17] = (moved[17][0], moved[17][1] + 0.5, *moved[17][2:])
    pod_moved = cases.box_scene(moved, planes=PLANE, spp=16)
    check_frame(tracer, pod_moved, 64, 36, 14, TREE, "bvh")
    assert tracer.kat_box_bvh_builds() == builds + 1
    check_frame(tracer, pod_moved, 64, 36, 15, TREE | SM, "bvh")
    assert tracer.kat_box_bvh_builds() == builds + 1
    with_sphere = cases.box_scene(moved, spheres=[(0, 0.7, 1.5, 0.4, 2)], planes=PLANE, spp=16)  # new columns, the same boxes
    check_frame(tracer, with_sphere, 64, 36, 14, TREE, "bvh")
    assert tracer.kat_box_bvh_builds() == builds + 1
    check_frame(tracer, pod, 64, 36, 14, TREE, "bvh")
    assert tracer.kat_box_bvh_builds() == builds + 2


def test_both_sphere_builders(tracer):
    from tests.test_gpu_boxes import grid_spheres

    pod = box_ref.scene_pod(cases.camera(), spheres=grid_spheres(200), planes=PLANE, boxes=cases.grid_boxes(300, pitch=0.3, half=0.1, z0=1.2), spp=16)
    for build in (capi.RT_HIP_FLAG_BVH, capi.RT_HIP_FLAG_BVH | capi.RT_HIP_FLAG_BVH_DEVICE_BUILD, 0):
        check_frame(tracer, pod, 64, 36, 16, TREE | build, "bvh")


def test_refusals_name_the_flag_and_launch_nothing(tracer):
    import torch

    pod = cases.box_scene(cases.grid_boxes(300, pitch=0.3, half=0.1, z0=1.0), planes=PLANE, spp=16)

    def refused_by_name(call, canvas=None):
        with pytest.raises(rt_amd.RtHipError) as refused:
            call()
        assert refused.value.status == UNSUPPORTED and "RT_HIP_FLAG_BOX_BVH" in str(refused.value), str(refused.value)
        assert canvas is None or (canvas == 0xDEADBEEF).all()

    for bit in (0, capi.RT_HIP_FLAG_FAST, capi.RT_HIP_FLAG_FORCE_TILED, capi.RT_HIP_FLAG_FORCE_RESIDENT, capi.RT_HIP_FLAG_FORCE_STREAMED, capi.RT_HIP_FLAG_FORCE_HALF_CHUNKS):
        canvas = np.full((36, 64), 0xDEADBEEF, dtype=np.uint32)
        flags = capi.RT_HIP_FLAG_BOX_BVH | bit | (BOXES if bit else 0)  # (bit 0: the flag without RT_HIP_FLAG_TRACE_BOXES)
        refused_by_name(lambda: tracer.render(pod, 64, 36, seed=1, flags=flags, out=canvas), canvas)
    refused_by_name(lambda: tracer.render_progressive(pod, 64, 36, seed=1, flags=TREE))
    refused_by_name(lambda: tracer.render_temporal(pod, 64, 36, seed=1, flags=TREE))
    tracer.upload(pod)
    accum = torch.zeros((36, 64, 3), dtype=torch.float32, device="cuda:0")
    frame = torch.full((36, 64), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    guide = torch.zeros((36, 64, 8), dtype=torch.float32, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    refused_by_name(lambda: tracer.render_pass_device(64, 36, 0, 16, accum.data_ptr(), frame.data_ptr(), flags=TREE))
    refused_by_name(lambda: tracer.render_device(64, 36, frame.data_ptr(), seed=1, flags=capi.RT_HIP_FLAG_BOX_BVH, stream=stream))
    refused_by_name(lambda: tracer.render_device(64, 36, frame.data_ptr(), seed=1, flags=TREE | capi.RT_HIP_FLAG_FAST, stream=stream))
    refused_by_name(lambda: tracer.guide_device(64, 36, guide.data_ptr(), flags=TREE, stream=stream))
    torch.cuda.synchronize()
    assert bool((frame == 0x5A5A5A5A).all()) and bool((accum == 0).all()) and bool((guide == 0).all())
    # the preview ignores it, and the context renders on
    preview = tracer.render(pod, 64, 36, seed=1, flags=capi.RT_HIP_FLAG_PREVIEW)
    flagged = tracer.render(pod, 64, 36, seed=1, flags=capi.RT_HIP_FLAG_PREVIEW | TREE)
    assert np.array_equal(preview[0], flagged[0]) and flagged[2]["kernel"] == "preview"
    check_frame(tracer, pod, 64, 36, 1, TREE, "bvh")
    assert rt_amd.live_frame_locks() == 0


def test_two_ranks_and_two_members(tracer):
    """rt_hip_render_device as ranks 0 and 1 of 2, and one frame through rt_hip_create_multi (two members on the device that is here)."""
    import torch

    width, height = 64, 36
    pod = cases.box_scene(cases.grid_boxes(300, pitch=0.3, half=0.1, z0=1.0), spheres=[(0, 0.7, 1.5, 0.4, 2)], planes=PLANE, spp=16)
    want_rgba, want_rgb, want = box_ref.render(pod, width, height, seed=17)
    tracer.upload(pod)
    padded = rt_amd.padded_local_rows(height, 2, 8)
    gathered = torch.zeros((2, padded, width), dtype=torch.int32, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    segments = 0
    for rank in range(2):
        tracer.render_device(width, height, gathered[rank].data_ptr(), seed=17, flags=TREE, partition=(rank, 2, 8), stream=stream)
        torch.cuda.synchronize()
        stats = tracer.stats()
        assert stats["kernel"] == "bvh"
        segments += stats["segments"]
        part, _, _ = box_ref.render(pod, width, height, seed=17, partition=(rank, 2, 8), want_rgb=False)
        assert np.array_equal(gathered[rank].cpu().numpy().view(np.uint32)[: part.shape[0]], part), rank
    assert segments == want["segments"]
    with rt_amd.HipRayTracer(devices=[0, 0], peer_copy=True) as multi:
        rgba, rgb, stats = multi.render(pod, width, height, seed=17, flags=TREE, want_rgb=True)
        assert np.array_equal(rgba, want_rgba) and np.array_equal(rgb.view(np.uint32), want_rgb.view(np.uint32)) and stats["segments"] == want["segments"]


def test_headless_renders_box_field(tmp_path):
    """rt_headless --boxes --box-bvh on tests/golden/scenes/box_field.toml (304 boxes) equals the restatement's frame; --boxes alone is
    refused by the module for the box count, --box-bvh alone by the driver."""
    binary = ROOT / "rt_amd" / "bin" / "rt_headless"
    scene_file = GOLDEN / "scenes" / "box_field.toml"
    run = lambda *args: subprocess.run([str(binary), *args], cwd=ROOT, capture_output=True, text=True, timeout=300)  # noqa: E731
    ppm = tmp_path / "field.ppm"
    out = run("--renderer", "hip", "--scene", str(scene_file), "--size", "64x36", "--spp", "16", "--seed", "5", "--boxes", "--box-bvh", "--out", str(ppm))
    assert out.returncode == 0 and "error:" not in out.stderr, out.stderr
    header = b"P6\n64 36\n255\n"
    got = np.frombuffer(ppm.read_bytes()[len(header) :], dtype=np.uint8).reshape(36, 64, 3)
    pod = rt_amd.Scene.load(scene_file).set_sampling(16).describe(64, 36)
    assert pod.n_boxes == 304
    want, _, _ = box_ref.render(pod, 64, 36, seed=5, want_rgb=False)
    assert np.array_equal(got, unpack(want)[..., :3])
    out = run("--renderer", "hip", "--scene", str(scene_file), "--size", "64x36", "--box-bvh")
    assert out.returncode == 2 and "--box-bvh" in out.stderr
    out = run("--renderer", "hip", "--scene", str(scene_file), "--size", "64x36", "--spp", "16", "--boxes")
    assert "304 boxes" in out.stderr
