"""RT_HIP_FLAG_TRACE_BOXES on the GPU: every frame is compared bit for bit — packed pixels, float mean, segments — with
the CPU restatement of the box contract (tests/native/box_reference.cpp: the frozen oracle with a test_boxes that hits), and the
kernel that ran is checked.  Tolerance 0 everywhere.  The cases walk the eight box builds: the resident kernel's LDS scan through a
pinhole and through a tilted camera, its scalar-load scan, the hierarchy kernel with both builders and by the scene's size — each
with the mg and the sm table where the scene has a material that tells them apart."""
import numpy as np
import pytest

import rt_amd
from oracle import binding as oracle
from rt_amd import capi
from tests import box_reference as box_ref
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu

BOXES = capi.RT_HIP_FLAG_TRACE_BOXES
SM = capi.RT_HIP_FLAG_SM_MATERIALS
UNSUPPORTED = 5


def check_frame(tracer, pod, width, height, seed, flags, kernel, partition=None):
    """rt_hip_render with `flags` against box_ref_render: rgba8, rgb_f32, segments; kernel_variant."""
    rgba, rgb, stats = tracer.render(pod, width, height, seed=seed, flags=flags, want_rgb=True)
    want_rgba, want_rgb, want = box_ref.render(pod, width, height, seed=seed, sm_materials=bool(flags & SM))
    assert stats["kernel"] == kernel, stats
    assert np.array_equal(rgba, want_rgba), f"{(rgba != want_rgba).sum()} of {rgba.size} pixels differ from the restatement's"
    assert np.array_equal(rgb.view(np.uint32), want_rgb.view(np.uint32))
    assert stats["segments"] == want["segments"]
    return rgba, stats


def boxes_scene(position=None, direction=None, spp=20):
    scene = rt_amd.Scene.load(GOLDEN / "scenes" / "boxes.toml").set_sampling(spp)
    if position is not None:
        scene.set_camera(position, direction)
    return scene


@pytest.mark.parametrize("table", [0, SM])
@pytest.mark.parametrize("camera,form", [(((0.5, 1.6, 5.5), (0, 0, -1)), "pinhole"), (((0.5, 1.6, 5.5), (0.3, -0.25, -1)), "eye")])
def test_boxes_toml(tracer, table, camera, form):
    """1. The scene of the flag, both tables, through an axis-aligned and a tilted camera: both LDS-scan builds."""
    scene = boxes_scene(*camera)
    pod = scene.describe(96, 54)
    assert oracle.primary_ray(pod, 96, 54, 0, 0, want_form=True)[2] == form
    rgba, _ = check_frame(tracer, pod, 96, 54, 11, BOXES | table, "resident")
    flat, _, _ = oracle.render(pod, 96, 54, seed=11, want_rgb=False, sm_materials=bool(table))
    assert (rgba != flat).mean() > 0.05  # the boxes are in the frame


def test_the_golden_box_frame(tracer):
    golden = np.load(GOLDEN / "boxes_64x36_spp20.npz")
    pod = boxes_scene().set_sampling(int(golden["spp"]), int(golden["max_bounces"])).describe(64, 36)
    for table, suffix in ((0, ""), (SM, "_sm")):
        rgba, _, stats = tracer.render(pod, 64, 36, seed=int(golden["seed"]), flags=BOXES | table)
        assert np.array_equal(rgba, golden["rgba" + suffix]) and stats["segments"] == int(golden["segments" + suffix])


@pytest.fixture(scope="module")
def camera():
    return rt_amd.Scene.named("basic").describe(64, 36)


def test_boxes_only(tracer, camera):
    """2. No sphere, no plane, three boxes."""
    pod = box_ref.scene_pod(camera, boxes=[(-1.2, 0.5, 0, 0.5, 0.5, 0.5, 0), (0.2, 0.4, -1, 0.6, 0.4, 0.3, 1), (1.3, 0.8, 0.5, 0.3, 0.8, 0.3, 2)])
    for table in (0, SM):
        check_frame(tracer, pod, 64, 36, 3, BOXES | table, "resident")


def test_camera_inside_a_hollow_looking_box(tracer, camera):
    """3. Every primary ray starts inside box 0 and meets an exit face (outward normal, never flipped) unless the sphere is in the way."""
    pod = box_ref.scene_pod(camera, spheres=[(0, 0.5, 0, 0.5, 1), (1.2, 0.6, 0.5, 0.4, 2)], boxes=[(0, 1, 0, 8, 4, 8, 3)])
    t, kind, _, normal = box_ref.closest_hit(pod, [(0, 1, 3)], [(0, 0, -1)])
    assert kind[0] == 1  # (the sphere, straight ahead of basic.toml's camera at (0, 1, 3))
    t, kind, _, normal = box_ref.closest_hit(pod, [(0, 1, 3)], [(0, 1, 0)])
    assert kind[0] == 3 and t[0] == 4.0 and tuple(normal[0]) == (0.0, 1.0, 0.0)
    for table in (0, SM):
        check_frame(tracer, pod, 64, 36, 4, BOXES | table, "resident")


def grid_spheres(count, radius=0.12, pitch=0.3, material_count=4):
    side = int(np.ceil(np.sqrt(count)))
    return [((i % side - side / 2) * pitch, radius, -(i // side) * pitch, radius, i % material_count) for i in range(count)]


def test_the_scalar_load_build(tracer, camera):
    """4. 45 spheres (the scalar-load scan starts at 40), 5 boxes, 1 plane."""
    boxes = [(-1.5 + 0.7 * i, 0.3 + 0.1 * i, 0.8, 0.2, 0.3 + 0.1 * i, 0.2, i % 4) for i in range(5)]
    pod = box_ref.scene_pod(camera, spheres=grid_spheres(45), planes=[(0, 1, 0, 0, 0)], boxes=boxes)
    for table in (0, SM):
        check_frame(tracer, pod, 64, 36, 5, BOXES | table, "resident")


@pytest.mark.parametrize("build", [0, capi.RT_HIP_FLAG_BVH_DEVICE_BUILD])
def test_the_hierarchy_build_with_the_flag(tracer, camera, build):
    """5a. 200 spheres and 7 boxes under RT_HIP_FLAG_BVH, the host's tree and the device builder's."""
    boxes = [(-1.8 + 0.6 * i, 0.25 + 0.05 * i, 1.0, 0.2, 0.25 + 0.05 * i, 0.2, i % 4) for i in range(7)]
    pod = box_ref.scene_pod(camera, spheres=grid_spheres(200), planes=[(0, 1, 0, 0, 0)], boxes=boxes)
    for table in (0, SM):
        check_frame(tracer, pod, 64, 36, 6, BOXES | capi.RT_HIP_FLAG_BVH | build | table, "bvh")


def test_a_scene_of_the_streamed_kernels_size_is_planned_onto_the_hierarchy(tracer):
    """5b. 1 400 spheres and 2 boxes without RT_HIP_FLAG_BVH, 32x18x16."""
    camera = rt_amd.Scene.named("basic").describe(32, 18)
    pod = box_ref.scene_pod(camera, spheres=grid_spheres(1400, radius=0.05, pitch=0.12), boxes=[(-0.8, 0.5, 1, 0.3, 0.5, 0.3, 1), (0.9, 0.3, 1.2, 0.3, 0.3, 0.3, 2)], spp=16)
    _, _, flagless = tracer.render(pod, 32, 18, seed=7)
    assert flagless["kernel"] == "streamed"
    check_frame(tracer, pod, 32, 18, 7, BOXES, "bvh")


def test_256_boxes_fill_the_last_lds_slot(tracer):
    """6. A 16 x 16 grid of boxes, 32x18x16: the launch takes the plan's LDS bytes, the last pair of float4s included (box 255 is the
    one straight ahead of the camera, nearer than every other)."""
    camera = rt_amd.Scene.named("basic").describe(32, 18)
    boxes = [((i % 16 - 7.5) * 0.5, (i // 16) * 0.3 - 1.0, -3.0, 0.2, 0.12, 0.2, i % 4) for i in range(255)] + [(0, 1, 1.5, 0.3, 0.3, 0.3, 1)]
    pod = box_ref.scene_pod(camera, boxes=boxes, spp=16)
    _, kind, index, _ = box_ref.closest_hit(pod, [(0, 1, 3)], [(0, 0, -1)])
    assert kind[0] == 3 and index[0] == 255
    check_frame(tracer, pod, 32, 18, 8, BOXES, "resident")


def test_without_a_box_the_flag_changes_nothing(tracer):
    """7. basic.toml: frame, segments and kernel_variant of the flagless call."""
    pod = rt_amd.Scene.named("basic").set_sampling(20).describe(64, 36)
    plain = tracer.render(pod, 64, 36, seed=9, want_rgb=True)
    flagged = tracer.render(pod, 64, 36, seed=9, flags=BOXES, want_rgb=True)
    assert np.array_equal(plain[0], flagged[0]) and np.array_equal(plain[1].view(np.uint32), flagged[1].view(np.uint32))
    assert (plain[2]["kernel"], plain[2]["segments"]) == (flagged[2]["kernel"], flagged[2]["segments"]) and plain[2]["kernel"] == "small"
    want, _, _ = oracle.render(pod, 64, 36, seed=9, want_rgb=False)
    assert np.array_equal(plain[0], want)


def test_without_the_flag_boxes_toml_is_the_oracles_frame(tracer):
    """8. Today's behaviour, unchanged: the boxes reach the module and the traced frame does not show them."""
    pod = boxes_scene().describe(64, 36)
    rgba, rgb, stats = tracer.render(pod, 64, 36, seed=10, want_rgb=True)
    want_rgba, want_rgb, want = oracle.render(pod, 64, 36, seed=10)
    assert np.array_equal(rgba, want_rgba) and np.array_equal(rgb.view(np.uint32), want_rgb.view(np.uint32)) and stats["segments"] == want["segments"]
    assert stats["kernel"] == "small"


def test_two_ranks_assemble_the_whole_frame(tracer):
    """9. rt_hip_render_device as ranks 0 and 1 of 2."""
    import torch

    width, height = 96, 54
    pod = boxes_scene().describe(width, height)
    whole, _, whole_stats = tracer.render(pod, width, height, seed=12, flags=BOXES)
    tracer.upload(pod)
    padded = rt_amd.padded_local_rows(height, 2, 8)
    gathered = torch.zeros((2, padded, width), dtype=torch.int32, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    segments = 0
    for rank in range(2):
        tracer.render_device(width, height, gathered[rank].data_ptr(), seed=12, flags=BOXES, partition=(rank, 2, 8), stream=stream)
        torch.cuda.synchronize()
        stats = tracer.stats()
        assert stats["kernel"] == "resident"
        segments += stats["segments"]
        part, _, _ = box_ref.render(pod, width, height, seed=12, partition=(rank, 2, 8), want_rgb=False)
        assert np.array_equal(gathered[rank].cpu().numpy().view(np.uint32)[: part.shape[0]], part), rank
    frame = torch.empty((height, width), dtype=torch.int32, device="cuda:0")
    tracer.assemble_device(width, height, 2, 8, gathered.data_ptr(), frame.data_ptr(), stream)
    torch.cuda.synchronize()
    assert np.array_equal(frame.cpu().numpy().view(np.uint32), whole) and segments == whole_stats["segments"]


def test_the_device_query_equals_the_restatement(tracer, camera):
    """10. rt_hip_kat_closest_hit_boxes on the CPU tests' ray set (the hand-made rays and random ones aimed at the boxes)."""
    pod = box_ref.scene_pod(camera, box_ref.KAT_SPHERES, box_ref.KAT_PLANES, box_ref.KAT_BOXES)
    origins, directions, _ = box_ref.known_answer_rays()
    rng = np.random.default_rng(3)
    more_o = rng.uniform(-12, 12, (2000, 3)).astype(np.float32)
    aims = np.where(rng.integers(2, size=(2000, 1)) == 0, rng.uniform(-1, 1, (2000, 3)) * (1, 2, 3), rng.uniform(-1, 1, (2000, 3)) + (10, 2, 0))
    more_d = aims - more_o
    more_d = (more_d / np.linalg.norm(more_d, axis=1, keepdims=True)).astype(np.float32)
    origins, directions = np.concatenate([origins, more_o]), np.concatenate([directions, more_d])
    tracer.upload(pod)
    got = tracer.kat_closest_hit(origins, directions, boxes=True)
    want = box_ref.closest_hit(pod, origins, directions)
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))
    assert np.array_equal(got[3].view(np.uint32), want[3].view(np.uint32))
    assert (want[1] == 3).sum() > 500


def test_refusals_name_the_flag_and_launch_nothing(tracer, camera):
    """11. RT_HIP_UNSUPPORTED with the flag's name; the context renders on afterwards."""
    import torch

    pod = boxes_scene().describe(64, 36)
    for bit in (capi.RT_HIP_FLAG_FAST, capi.RT_HIP_FLAG_FORCE_TILED, capi.RT_HIP_FLAG_FORCE_RESIDENT, capi.RT_HIP_FLAG_FORCE_STREAMED, capi.RT_HIP_FLAG_FORCE_HALF_CHUNKS):
        canvas = np.full((36, 64), 0xDEADBEEF, dtype=np.uint32)
        with pytest.raises(rt_amd.RtHipError) as refused:
            tracer.render(pod, 64, 36, seed=1, flags=BOXES | bit, out=canvas)
        assert refused.value.status == UNSUPPORTED and "RT_HIP_FLAG_TRACE_BOXES" in str(refused.value)
        assert (canvas == 0xDEADBEEF).all()
    with pytest.raises(rt_amd.RtHipError) as refused:
        tracer.render_progressive(pod, 64, 36, seed=1, flags=BOXES)
    assert refused.value.status == UNSUPPORTED and "RT_HIP_FLAG_TRACE_BOXES" in str(refused.value)
    tracer.upload(pod)
    accum = torch.zeros((36, 64, 3), dtype=torch.float32, device="cuda:0")
    frame = torch.full((36, 64), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    with pytest.raises(rt_amd.RtHipError) as refused:
        tracer.render_pass_device(64, 36, 0, 16, accum.data_ptr(), frame.data_ptr(), flags=BOXES)
    assert refused.value.status == UNSUPPORTED and "RT_HIP_FLAG_TRACE_BOXES" in str(refused.value)
    torch.cuda.synchronize()
    assert bool((frame == 0x5A5A5A5A).all()) and bool((accum == 0).all())
    many = box_ref.scene_pod(camera, boxes=[(i * 0.01, 0, -5, 0.004, 0.1, 0.1, 0) for i in range(257)])
    canvas = np.full((36, 64), 0xDEADBEEF, dtype=np.uint32)
    with pytest.raises(rt_amd.RtHipError) as refused:
        tracer.render(many, 64, 36, seed=1, flags=BOXES, out=canvas)
    assert refused.value.status == UNSUPPORTED and "257 boxes" in str(refused.value) and (canvas == 0xDEADBEEF).all()
    tracer.render(many, 64, 36, seed=1)  # (without the flag the same scene renders)
    check_frame(tracer, pod, 64, 36, 1, BOXES, "resident")
    assert rt_amd.live_frame_locks() == 0  # 12. (the suite asserts it after every GPU test too)
