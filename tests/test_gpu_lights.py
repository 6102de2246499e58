"""RT_HIP_FLAG_EMISSION on the GPU: every frame is compared bit for bit — packed pixels, float mean, segments — with the
CPU restatement of the light contract (tests/native/light_reference.cpp: the frozen oracle with a trace loop that knows lights), and the
kernel that ran is checked.  Tolerance 0 everywhere.  The cases walk the eight light builds: the resident kernel's LDS scan through a
pinhole and through a tilted camera, its scalar-load scan, the hierarchy kernel with both builders and by the scene's size — each with
the mg and the sm table."""
import numpy as np
import pytest

import rt_amd
from oracle import binding as oracle
from rt_amd import capi
from tests import light_reference as light_ref
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu

EMISSION = capi.RT_HIP_FLAG_EMISSION
SM = capi.RT_HIP_FLAG_SM_MATERIALS
INVALID_ARGUMENT, UNSUPPORTED = 1, 5


@pytest.fixture(autouse=True)
def _no_table_outlives_a_test(tracer):
    yield
    tracer.set_emission(None)  # (the session's context is shared: no other test file sees a table)


def check_frame(tracer, pod, width, height, seed, flags, kernel, table):
    """rt_hip_render with `flags` under `table` against light_ref_render: rgba8, rgb_f32, segments; kernel_variant."""
    tracer.set_emission(table)
    rgba, rgb, stats = tracer.render(pod, width, height, seed=seed, flags=flags, want_rgb=True)
    want_rgba, want_rgb, want = light_ref.render(pod, width, height, table, seed=seed, sm_materials=bool(flags & SM))
    assert stats["kernel"] == kernel, stats
    assert np.array_equal(rgba, want_rgba), f"{(rgba != want_rgba).sum()} of {rgba.size} pixels differ from the restatement's"
    assert np.array_equal(rgb.view(np.uint32), want_rgb.view(np.uint32))
    assert stats["segments"] == want["segments"]
    return rgba, rgb, stats


@pytest.mark.parametrize("table", [0, SM])
@pytest.mark.parametrize("camera,form", [(((0.3, 1.5, 5.0), (0, 0, -1)), "pinhole"), (((0.3, 1.5, 5.0), (0.2, -0.15, -1)), "eye")])
def test_lights_toml(tracer, table, camera, form):
    """1. The scene of the flag, both tables, through an axis-aligned and a tilted camera: both LDS-scan builds."""
    pod = light_ref.lights_scene(*camera).describe(96, 54)
    assert oracle.primary_ray(pod, 96, 54, 0, 0, want_form=True)[2] == form
    rgba, _, _ = check_frame(tracer, pod, 96, 54, 11, EMISSION | table, "resident", light_ref.LIGHTS_TABLE)
    flat, _, _ = oracle.render(pod, 96, 54, seed=11, want_rgb=False, sm_materials=bool(table))
    assert (rgba != flat).mean() > 0.05  # the lamp lights the frame


def test_the_golden_light_frame(tracer):
    """2. The committed frame, both tables."""
    golden = np.load(GOLDEN / "lights_64x36_spp20.npz")
    pod = light_ref.lights_scene(spp=int(golden["spp"]), bounces=int(golden["max_bounces"])).describe(64, 36)
    tracer.set_emission(golden["emission"])
    for table, suffix in ((0, ""), (SM, "_sm")):
        rgba, _, stats = tracer.render(pod, 64, 36, seed=int(golden["seed"]), flags=EMISSION | table)
        assert np.array_equal(rgba, golden["rgba" + suffix]) and stats["segments"] == int(golden["segments" + suffix])


def test_the_furnace(tracer):
    """3. spp 33 — two chunks and a tail of one: every pixel's float mean is exactly E, one segment per sample, blue clamped."""
    width, height, spp = 64, 36, 33
    pod, table = light_ref.furnace(width, height, spp)
    for flags in (EMISSION, EMISSION | SM):
        rgba, rgb, stats = check_frame(tracer, pod, width, height, 3, flags, "resident", table)
        assert np.array_equal(rgb.view(np.uint32), np.broadcast_to(np.array(light_ref.FURNACE_E, dtype=np.float32).view(np.uint32), rgb.shape))
        assert stats["segments"] == width * height * spp and (rgba & 0xFF00 == 0xFF00).all()


@pytest.fixture(scope="module")
def camera():
    return rt_amd.Scene.named("basic").describe(64, 36)


def every_fourth(n_materials=4, rgb=(2.0, 1.5, 1.0), which=3):
    table = np.zeros((n_materials, 3), dtype=np.float32)
    table[which] = rgb
    return table


def test_the_scalar_load_build(tracer, camera):
    """4. A grid of 48 spheres (the scalar-load scan starts at 40) whose every fourth material is a light, and a plane."""
    pod = light_ref.scene_pod(camera, spheres=light_ref.grid_spheres(48), planes=[(0, 1, 0, 0, 0)])
    for table in (0, SM):
        check_frame(tracer, pod, 64, 36, 5, EMISSION | table, "resident", every_fourth())


@pytest.mark.parametrize("build", [0, capi.RT_HIP_FLAG_BVH_DEVICE_BUILD])
def test_the_hierarchy_build_with_the_flag(tracer, camera, build):
    """5a. 200 spheres under RT_HIP_FLAG_BVH, the host's tree and the device builder's."""
    pod = light_ref.scene_pod(camera, spheres=light_ref.grid_spheres(200), planes=[(0, 1, 0, 0, 0)])
    for table in (0, SM):
        check_frame(tracer, pod, 64, 36, 6, EMISSION | capi.RT_HIP_FLAG_BVH | build | table, "bvh", every_fourth(which=1))


def test_a_scene_of_the_streamed_kernels_size_is_planned_onto_the_hierarchy(tracer):
    """5b. 1301 spheres without RT_HIP_FLAG_BVH, 32x18x16."""
    camera = rt_amd.Scene.named("basic").describe(32, 18)
    pod = light_ref.scene_pod(camera, spheres=light_ref.grid_spheres(1301, radius=0.05, pitch=0.12), spp=16)
    _, _, flagless = tracer.render(pod, 32, 18, seed=7)
    assert flagless["kernel"] == "streamed"
    check_frame(tracer, pod, 32, 18, 7, EMISSION, "bvh", every_fourth(which=2))


def test_a_light_plane_and_tables_of_every_shape(tracer, camera):
    """6. A ceiling that is a light over one lambert sphere (a plane hit from below: a light is not sided); every material a light; only
    material 0; only the last one."""
    ceiling = light_ref.scene_pod(camera, spheres=[(0, 0.5, 0, 0.5, 3)], planes=[(0, 1, 0, 0, 0), (0, 1, 0, -4, 1)])
    check_frame(tracer, ceiling, 64, 36, 12, EMISSION, "resident", every_fourth(which=1, rgb=(1.5, 1.5, 1.25)))
    pod = light_ref.scene_pod(camera, spheres=[(-1.2, 0.5, 0, 0.5, 0), (0, 0.5, -1, 0.5, 1), (1.2, 0.5, 0, 0.5, 2), (0.3, 0.3, 1.2, 0.3, 3)], planes=[(0, 1, 0, 0, 3)])
    everything = np.array([(1, 0.5, 0.25), (0.5, 1, 0.25), (0.25, 0.5, 1), (0.125, 0.125, 0.125)], dtype=np.float32)
    for table in (everything, every_fourth(which=0), every_fourth(which=3)):
        for sm in (0, SM):
            check_frame(tracer, pod, 64, 36, 13, EMISSION | sm, "resident", table)


@pytest.mark.parametrize("spp", [16, 17])
def test_one_chunk_and_a_tail_of_one(tracer, spp):
    """7a. spp 16 and 17."""
    pod = light_ref.lights_scene(spp=spp).describe(64, 36)
    check_frame(tracer, pod, 64, 36, 14, EMISSION, "resident", light_ref.LIGHTS_TABLE)


def test_one_bounce(tracer):
    """7b. max_bounces = 1: a path with no bounce left is worth 0 before it can reach a light."""
    pod = light_ref.lights_scene(bounces=1).describe(64, 36)
    for sm in (0, SM):
        check_frame(tracer, pod, 64, 36, 15, EMISSION | sm, "resident", light_ref.LIGHTS_TABLE)


def test_a_lamp_of_1000(tracer, camera):
    """7c. One small sphere with E = 1000: the float mean is far above 1 and bit-exact, the packed pixel clamps."""
    pod = light_ref.scene_pod(camera, spheres=[(0, 1, 0, 0.3, 1), (0.8, 0.5, 0.5, 0.5, 0)], planes=[(0, 1, 0, 0, 3)])
    rgba, rgb, _ = check_frame(tracer, pod, 64, 36, 16, EMISSION, "resident", every_fourth(which=1, rgb=(1000, 1000, 1000)))
    assert rgb.max() == 1000.0 and (rgb > 1.0).any(axis=2).sum() > 20
    assert (rgba[(rgb > 1.0).all(axis=2)] == 0xFFFFFFFF).all()


def test_without_a_light_the_flag_changes_nothing(tracer):
    """8. basic.toml with the flag and an all-zero table: frame, segments and kernel_variant of the flag-less call, which is the oracle's."""
    pod = rt_amd.Scene.named("basic").set_sampling(20).describe(64, 36)
    plain = tracer.render(pod, 64, 36, seed=9, want_rgb=True)
    tracer.set_emission(np.zeros((pod.n_materials, 3), dtype=np.float32))
    flagged = tracer.render(pod, 64, 36, seed=9, flags=EMISSION, want_rgb=True)
    assert np.array_equal(plain[0], flagged[0]) and np.array_equal(plain[1].view(np.uint32), flagged[1].view(np.uint32))
    assert (plain[2]["kernel"], plain[2]["segments"]) == (flagged[2]["kernel"], flagged[2]["segments"]) and plain[2]["kernel"] == "small"
    want, _, _ = oracle.render(pod, 64, 36, seed=9, want_rgb=False)
    assert np.array_equal(plain[0], want)


def test_without_the_flag_a_table_changes_nothing(tracer):
    """9. A table with lights and no flag: the oracle's frame."""
    pod = light_ref.lights_scene().describe(64, 36)
    tracer.set_emission(light_ref.LIGHTS_TABLE)
    rgba, rgb, stats = tracer.render(pod, 64, 36, seed=10, want_rgb=True)
    want_rgba, want_rgb, want = oracle.render(pod, 64, 36, seed=10)
    assert np.array_equal(rgba, want_rgba) and np.array_equal(rgb.view(np.uint32), want_rgb.view(np.uint32)) and stats["segments"] == want["segments"]
    assert stats["kernel"] == "small"


def test_the_table_is_context_state(tracer, camera):
    """10. Same scene, same fingerprint, the table replaced between two frames: the second frame follows the new table.  Cleared: the
    flag is refused.  The scene replaced by one with another material count: refused, with both counts in the message."""
    pod = light_ref.lights_scene().describe(64, 36)
    first, _, _ = check_frame(tracer, pod, 64, 36, 17, EMISSION, "resident", light_ref.LIGHTS_TABLE)
    other = np.zeros((5, 3), dtype=np.float32)
    other[2] = (0.5, 2, 0.5)  # the clay sphere glows instead
    second, _, _ = check_frame(tracer, pod, 64, 36, 17, EMISSION, "resident", other)
    assert (first != second).mean() > 0.05
    again, _, _ = check_frame(tracer, pod, 64, 36, 17, EMISSION, "resident", light_ref.LIGHTS_TABLE)
    assert np.array_equal(first, again)
    before = tracer.stats()
    tracer.set_emission(None)
    canvas = np.full((36, 64), 0xDEADBEEF, dtype=np.uint32)
    with pytest.raises(rt_amd.RtHipError) as refused:
        tracer.render(pod, 64, 36, seed=17, flags=EMISSION, out=canvas)
    assert refused.value.status == INVALID_ARGUMENT and "RT_HIP_FLAG_EMISSION" in str(refused.value) and (canvas == 0xDEADBEEF).all()
    tracer.set_emission(light_ref.LIGHTS_TABLE)  # five rows; the next scene has four materials
    four = light_ref.scene_pod(camera, spheres=[(0, 0.5, 0, 0.5, 1)], planes=[(0, 1, 0, 0, 0)])
    with pytest.raises(rt_amd.RtHipError) as refused:
        tracer.render(four, 64, 36, seed=17, flags=EMISSION, out=canvas)
    assert refused.value.status == INVALID_ARGUMENT and "5 rows" in str(refused.value) and "4 materials" in str(refused.value) and (canvas == 0xDEADBEEF).all()
    after = tracer.stats()
    assert (after["segments"], after["kernel"], after["primary_samples"]) == (before["segments"], before["kernel"], before["primary_samples"])
    check_frame(tracer, four, 64, 36, 17, EMISSION, "resident", every_fourth(which=1))  # (the table survives nothing it should not: a fitting one renders)
    with pytest.raises(rt_amd.RtHipError) as refused:
        tracer.set_emission([(0, 0, 0), (1, float("nan"), 0)])
    assert refused.value.status == INVALID_ARGUMENT and "material 1, component g" in str(refused.value)
    for bad in (-1.0, float("inf")):
        with pytest.raises(rt_amd.RtHipError) as refused:
            tracer.set_emission([(0, 0, bad)])
        assert refused.value.status == INVALID_ARGUMENT and "material 0, component b" in str(refused.value)
    check_frame(tracer, four, 64, 36, 18, EMISSION, "resident", every_fourth(which=1))  # (a refused table left the old one in place)


def test_two_ranks_assemble_the_whole_frame(tracer):
    """11a. rt_hip_render_device as ranks 0 and 1 of 2."""
    import torch

    width, height = 96, 54
    pod = light_ref.lights_scene().describe(width, height)
    tracer.set_emission(light_ref.LIGHTS_TABLE)
    whole, _, whole_stats = tracer.render(pod, width, height, seed=12, flags=EMISSION)
    tracer.upload(pod)
    padded = rt_amd.padded_local_rows(height, 2, 8)
    gathered = torch.zeros((2, padded, width), dtype=torch.int32, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    segments = 0
    for rank in range(2):
        tracer.render_device(width, height, gathered[rank].data_ptr(), seed=12, flags=EMISSION, partition=(rank, 2, 8), stream=stream)
        torch.cuda.synchronize()
        stats = tracer.stats()
        assert stats["kernel"] == "resident"
        segments += stats["segments"]
        part, _, _ = light_ref.render(pod, width, height, light_ref.LIGHTS_TABLE, seed=12, partition=(rank, 2, 8), want_rgb=False)
        assert np.array_equal(gathered[rank].cpu().numpy().view(np.uint32)[: part.shape[0]], part), rank
    frame = torch.empty((height, width), dtype=torch.int32, device="cuda:0")
    tracer.assemble_device(width, height, 2, 8, gathered.data_ptr(), frame.data_ptr(), stream)
    torch.cuda.synchronize()
    assert np.array_equal(frame.cpu().numpy().view(np.uint32), whole) and segments == whole_stats["segments"]


def test_a_multi_gpu_context_hands_the_table_to_every_member():
    """11b. rt_hip_create_multi with two members — over two devices where two are visible, else twice the one device (peer copies, as
    tests/test_gpu_multi.py does): the table set on the context reaches both, and the assembled frame is the whole frame."""
    width, height = 96, 54
    pod = light_ref.lights_scene().describe(width, height)
    want_rgba, _, want = light_ref.render(pod, width, height, light_ref.LIGHTS_TABLE, seed=19, want_rgb=False)
    two = rt_amd.renderer.device_count() >= 2
    with rt_amd.HipRayTracer(devices=[0, 1] if two else [0, 0], peer_copy=not two) as multi:
        multi.set_emission(light_ref.LIGHTS_TABLE)
        rgba, _, stats = multi.render(pod, width, height, seed=19, flags=EMISSION)
        assert np.array_equal(rgba, want_rgba) and stats["segments"] == want["segments"]
        assert all(multi.member_stats(rank)["kernel"] == "resident" for rank in range(2))


def test_refusals_name_the_flag_and_launch_nothing(tracer):
    """12. Every refusal through the real entry points: the stated status, the flag's name in the message, and afterwards
    rt_hip_stats_fetch still returns the previous frame's counters — nothing was launched."""
    import torch

    pod = light_ref.lights_scene().describe(64, 36)
    check_frame(tracer, pod, 64, 36, 1, EMISSION, "resident", light_ref.LIGHTS_TABLE)
    before = tracer.stats()

    def nothing_ran():
        now = tracer.stats()
        return (now["segments"], now["kernel"], now["primary_samples"]) == (before["segments"], before["kernel"], before["primary_samples"])

    def refused_by_name(call, status=UNSUPPORTED):
        with pytest.raises(rt_amd.RtHipError) as refused:
            call()
        assert refused.value.status == status and "RT_HIP_FLAG_EMISSION" in str(refused.value), str(refused.value)
        assert nothing_ran()

    for bit in (capi.RT_HIP_FLAG_FAST, capi.RT_HIP_FLAG_FORCE_TILED, capi.RT_HIP_FLAG_FORCE_RESIDENT, capi.RT_HIP_FLAG_FORCE_STREAMED, capi.RT_HIP_FLAG_FORCE_HALF_CHUNKS, capi.RT_HIP_FLAG_TRACE_BOXES,
                capi.RT_HIP_FLAG_TRACE_BOXES | capi.RT_HIP_FLAG_BOX_BVH):
        canvas = np.full((36, 64), 0xDEADBEEF, dtype=np.uint32)
        refused_by_name(lambda: tracer.render(pod, 64, 36, seed=1, flags=EMISSION | bit, out=canvas))
        assert (canvas == 0xDEADBEEF).all()
    for bit in (12, 15, 20, 31):  # unassigned bits keep their answer
        with pytest.raises(rt_amd.RtHipError) as refused:
            tracer.render(pod, 64, 36, seed=1, flags=EMISSION | (1 << bit))
        assert refused.value.status == UNSUPPORTED and "unknown flag bits" in str(refused.value)
    refused_by_name(lambda: tracer.render_progressive(pod, 64, 36, seed=1, flags=EMISSION))
    refused_by_name(lambda: tracer.render_adaptive(pod, 64, 36, seed=1, flags=EMISSION))
    refused_by_name(lambda: tracer.render_temporal(pod, 64, 36, seed=1, flags=EMISSION))
    tracer.upload(pod)
    accum = torch.zeros((36, 64, 3), dtype=torch.float32, device="cuda:0")
    block = torch.zeros((9, 36, 64), dtype=torch.float32, device="cuda:0")
    guide = torch.zeros((36, 64, 8), dtype=torch.float32, device="cuda:0")
    frame = torch.full((36, 64), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    refused_by_name(lambda: tracer.render_pass_device(64, 36, 0, 16, accum.data_ptr(), frame.data_ptr(), flags=EMISSION))
    refused_by_name(lambda: tracer.adaptive_pass_device(64, 36, 0, 16, block.data_ptr(), frame.data_ptr(), flags=EMISSION))
    refused_by_name(lambda: tracer.guide_device(64, 36, guide.data_ptr(), flags=EMISSION))
    tracer.set_emission(None)
    refused_by_name(lambda: tracer.render_device(64, 36, frame.data_ptr(), flags=EMISSION), INVALID_ARGUMENT)
    torch.cuda.synchronize()
    assert bool((frame == 0x5A5A5A5A).all()) and bool((accum == 0).all()) and bool((block == 0).all()) and bool((guide == 0).all())
    # (rt_hip_denoise_progressive takes no flags: it filters the accumulation rt_hip_render_progressive made, which refuses the flag above)
    check_frame(tracer, pod, 64, 36, 1, EMISSION, "resident", light_ref.LIGHTS_TABLE)  # the context renders on
    assert rt_amd.live_frame_locks() == 0
