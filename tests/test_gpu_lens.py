"""RT_HIP_FLAG_THIN_LENS on the GPU: every frame is compared bit for bit — packed pixels, float mean, segments — with the
CPU restatement of the lens contract (tests/native/lens_reference.cpp: the frozen oracle with a sample loop that knows a lens, over the
rules header the device runs), and the kernel that ran is checked.  Tolerance 0 everywhere.  The cases walk the eight lens builds: the
resident kernel's LDS scan through a pinhole and through the two eye forms, its scalar-load scan, the hierarchy kernel with both
builders and by the scene's size — each with the mg and the sm table."""
import numpy as np
import pytest

import rt_amd
from oracle import binding as oracle
from rt_amd import capi
from tests import bloom_reference as bloom_ref
from tests import lens_reference as lens_ref
from tests import test_sky_band_rule as band_rule
from tests import tonemap_reference as tonemap_ref
from tests.conftest import GOLDEN
from tests.test_sky_band_rule import dump  # noqa: F401  (the fixture: sky_band_dump built with g++)

pytestmark = pytest.mark.gpu

LENS_FLAG = capi.RT_HIP_FLAG_THIN_LENS
SM = capi.RT_HIP_FLAG_SM_MATERIALS
INVALID_ARGUMENT, UNSUPPORTED = 1, 5
LENS = (0.06, 3.4)


@pytest.fixture(autouse=True)
def _no_lens_outlives_a_test(tracer):
    yield
    tracer.set_lens(None)  # (the session's context is shared: no other test file sees a lens)


def check_frame(tracer, pod, width, height, seed, flags, kernel, lens=LENS):
    """rt_hip_render with `flags` under `lens` against lens_ref_render: rgba8, rgb_f32, segments; kernel_variant."""
    tracer.set_lens(*lens)
    rgba, rgb, stats = tracer.render(pod, width, height, seed=seed, flags=flags, want_rgb=True)
    want_rgba, want_rgb, want = lens_ref.render(pod, width, height, lens, seed=seed, sm_materials=bool(flags & SM))
    assert stats["kernel"] == kernel, stats
    assert np.array_equal(rgba, want_rgba), f"{(rgba != want_rgba).sum()} of {rgba.size} pixels differ from the restatement's"
    assert np.array_equal(rgb.view(np.uint32), want_rgb.view(np.uint32))
    assert stats["segments"] == want["segments"]
    return rgba, rgb, stats


camera_pod = lens_ref.camera_pod


@pytest.mark.parametrize("table", [0, SM])
@pytest.mark.parametrize("form", ["pinhole", "eye", "guarded"])
@pytest.mark.parametrize("name", ["basic", "dielectric"])
def test_the_reference_scenes_through_three_cameras(tracer, name, form, table):
    """1. basic.toml and dielectric.toml at 20 spp, both tables, through an axis-aligned, a tilted and a guarded-eye camera: both LDS-scan
    builds, every camera form a lens frame can have."""
    pod = camera_pod(name, form)
    rgba, _, _ = check_frame(tracer, pod, 64, 36, 11, LENS_FLAG | table, "resident")
    sharp, _, _ = oracle.render(pod, 64, 36, seed=11, want_rgb=False, sm_materials=bool(table))
    assert (rgba != sharp).mean() > 0.2  # the lens blurs the frame


def test_the_golden_lens_frame(tracer):
    """2. The committed frame, both tables."""
    golden = np.load(GOLDEN / "lens_64x36_spp20.npz")
    pod = lens_ref.named_scene("basic", lens_ref.AXIS_CAMERA, int(golden["spp"]), int(golden["max_bounces"])).describe(64, 36)
    tracer.set_lens(float(golden["aperture_radius"]), float(golden["focus_distance"]))
    for table, suffix in ((0, ""), (SM, "_sm")):
        rgba, _, stats = tracer.render(pod, 64, 36, seed=int(golden["seed"]), flags=LENS_FLAG | table)
        assert np.array_equal(rgba, golden["rgba" + suffix]) and stats["segments"] == int(golden["segments" + suffix])


@pytest.fixture(scope="module")
def camera():
    return lens_ref.named_scene("basic", lens_ref.AXIS_CAMERA).describe(64, 36)


def test_the_scalar_load_build(tracer, camera):
    """3. A grid of 48 spheres (the scalar-load scan starts at 40) and a plane, through the pinhole and through the tilted camera."""
    tilted = lens_ref.named_scene("basic", lens_ref.TILTED_CAMERA).describe(64, 36)
    for through in (camera, tilted):
        pod = lens_ref.scene_pod(through, spheres=lens_ref.grid_spheres(48), planes=[(0, 1, 0, 0, 0)])
        for table in (0, SM):
            check_frame(tracer, pod, 64, 36, 5, LENS_FLAG | table, "resident")


@pytest.mark.parametrize("build", [0, capi.RT_HIP_FLAG_BVH_DEVICE_BUILD])
def test_the_hierarchy_build_with_the_flag(tracer, camera, build):
    """4a. 200 spheres under RT_HIP_FLAG_BVH, the host's tree and the device builder's."""
    pod = lens_ref.scene_pod(camera, spheres=lens_ref.grid_spheres(200), planes=[(0, 1, 0, 0, 0)])
    for table in (0, SM):
        check_frame(tracer, pod, 64, 36, 6, LENS_FLAG | capi.RT_HIP_FLAG_BVH | build | table, "bvh")


def test_a_scene_of_the_streamed_kernels_size_is_planned_onto_the_hierarchy(tracer):
    """4b. 1300 spheres and a plane without RT_HIP_FLAG_BVH, 32x18x16."""
    small = lens_ref.named_scene("basic", lens_ref.AXIS_CAMERA).describe(32, 18)
    pod = lens_ref.scene_pod(small, spheres=lens_ref.grid_spheres(1300, radius=0.05, pitch=0.12), planes=[(0, 1, 0, 0, 0)], spp=16)
    _, _, flagless = tracer.render(pod, 32, 18, seed=7)
    assert flagless["kernel"] == "streamed"
    check_frame(tracer, pod, 32, 18, 7, LENS_FLAG, "bvh")


@pytest.mark.parametrize("spp", [1, 16, 17, 33])
def test_sample_counts(tracer, spp):
    """5a. spp 1 — sample 0 alone: the lens step with no jitter step in front — one chunk, a tail of one, two chunks and a tail."""
    pod = camera_pod("basic", "pinhole", spp=spp)
    check_frame(tracer, pod, 64, 36, 14, LENS_FLAG, "resident")
    if spp == 1:
        check_frame(tracer, camera_pod("basic", "eye", spp=1), 64, 36, 14, LENS_FLAG | SM, "resident")


@pytest.mark.parametrize("size", [(1, 1), (63, 37)])
def test_frame_sizes(tracer, size):
    """5b. One pixel, and a frame ragged against every tile shape."""
    for form in ("pinhole", "eye"):
        pod = camera_pod("dielectric", form, *size)
        check_frame(tracer, pod, *size, 15, LENS_FLAG, "resident")


def test_one_bounce(tracer):
    """5c. max_bounces = 1."""
    pod = camera_pod("basic", "pinhole", bounces=1)
    for sm in (0, SM):
        check_frame(tracer, pod, 64, 36, 16, LENS_FLAG | sm, "resident")


def test_a_wild_lens(tracer):
    """5d. A radius of 1000 with a focus of 1e-3, and the reverse: wild rays are still the restatement's."""
    for form in ("pinhole", "guarded"):
        pod = camera_pod("basic", form)
        check_frame(tracer, pod, 64, 36, 17, LENS_FLAG, "resident", lens=(1000.0, 1e-3))
        check_frame(tracer, pod, 64, 36, 17, LENS_FLAG, "resident", lens=(1e-3, 1000.0))


def test_without_an_aperture_the_flag_changes_nothing(tracer):
    """6. basic.toml with the flag and a lens of radius 0: frame, float mean, segments and kernel_variant of the flag-less call, which is
    the oracle's — the scalar-register kernel, band and all."""
    pod = rt_amd.Scene.named("basic").set_sampling(20).describe(64, 36)
    plain = tracer.render(pod, 64, 36, seed=9, want_rgb=True)
    tracer.set_lens(0.0, 2.5)
    flagged = tracer.render(pod, 64, 36, seed=9, flags=LENS_FLAG, want_rgb=True)
    assert np.array_equal(plain[0], flagged[0]) and np.array_equal(plain[1].view(np.uint32), flagged[1].view(np.uint32))
    assert (plain[2]["kernel"], plain[2]["segments"], plain[2]["primary_samples"]) == (flagged[2]["kernel"], flagged[2]["segments"], flagged[2]["primary_samples"]) and plain[2]["kernel"] == "small"
    want, _, _ = oracle.render(pod, 64, 36, seed=9, want_rgb=False)
    assert np.array_equal(plain[0], want)


def test_without_the_flag_a_lens_changes_nothing(tracer):
    """7. A lens with an aperture and no flag: the oracle's frame."""
    pod = rt_amd.Scene.named("dielectric").set_sampling(20).describe(64, 36)
    tracer.set_lens(0.3, 2.0)
    rgba, rgb, stats = tracer.render(pod, 64, 36, seed=10, want_rgb=True)
    want_rgba, want_rgb, want = oracle.render(pod, 64, 36, seed=10)
    assert np.array_equal(rgba, want_rgba) and np.array_equal(rgb.view(np.uint32), want_rgb.view(np.uint32)) and stats["segments"] == want["segments"]
    assert stats["kernel"] == "small"


def test_the_band_is_not_taken(tracer, dump):  # noqa: F811
    """8. The flag-less frame of this scene gives its top 16 rows to the sky band; a small sphere lurks just above the frustum, close to the
    camera, where no ray from the eye can reach it.  Through a lens of radius 0.5 rays do: the restatement shows pixels in the band's
    rows that are no sky (max_bounces 1: a hit is black and the sky's red is at least 0.5, so a mean below 0.5 holds a hit) and that the
    scene without the sphere does not show.  The device's frame is the restatement's there."""
    size, lens = (64, 40), (0.5, 2.0)
    lurking = [0.0, 1.55, 2.6, 0.15, 0]
    visible = [band_rule.GROUND, [0.0, 0.5, -1.0, 0.5, 0]]

    def scene(spheres):
        pod = band_rule.scene_of(spheres, (0.0, 1.0, 3.0), (0.0, 0.0, -1.0), size)
        pod.samples_per_pixel, pod.max_bounces = 20, 1
        return pod

    pod = scene(visible + [lurking])
    rows = band_rule.band_rows(dump, pod, size)
    assert rows == 16
    want_rgba, want_rgb, _ = lens_ref.render(pod, *size, lens, seed=3)
    without_rgba, _, _ = lens_ref.render(scene(visible), *size, lens, seed=3, want_rgb=False)
    assert (want_rgb[:rows, :, 0] < 0.5).any() and (want_rgba[:rows] != without_rgba[:rows]).any()
    _, _, flagless = tracer.render(pod, *size, seed=3)
    assert flagless["kernel"] == "small"
    rgba, _, _ = check_frame(tracer, pod, *size, 3, LENS_FLAG, "resident", lens=lens)
    assert np.array_equal(rgba[:rows], want_rgba[:rows])


def test_the_lens_is_context_state(tracer, camera):
    """9. It survives an upload, is replaced between two frames and is cleared by NULL; a refused lens leaves the old one in place."""
    pod = camera_pod("basic", "pinhole")
    first, _, _ = check_frame(tracer, pod, 64, 36, 17, LENS_FLAG, "resident", lens=(0.05, 3.0))
    other = lens_ref.scene_pod(camera, spheres=[(0, 0.5, 0, 0.5, 1), (0.9, 0.3, 0.8, 0.3, 2)], planes=[(0, 1, 0, 0, 0)])
    tracer.upload(other)  # another scene: the lens stays
    rgba, rgb, stats = tracer.render(other, 64, 36, seed=17, flags=LENS_FLAG, want_rgb=True)
    want_rgba, want_rgb, want = lens_ref.render(other, 64, 36, (0.05, 3.0), seed=17)
    assert np.array_equal(rgba, want_rgba) and np.array_equal(rgb.view(np.uint32), want_rgb.view(np.uint32)) and stats["segments"] == want["segments"]
    second, _, _ = check_frame(tracer, pod, 64, 36, 17, LENS_FLAG, "resident", lens=(0.2, 1.5))
    assert (first != second).mean() > 0.05
    again, _, _ = check_frame(tracer, pod, 64, 36, 17, LENS_FLAG, "resident", lens=(0.05, 3.0))
    assert np.array_equal(first, again)
    for bad, field in (((float("nan"), 1.0), "aperture_radius"), ((-1.0, 1.0), "aperture_radius"), ((0.1, 0.0), "focus_distance"), ((0.1, float("inf")), "focus_distance")):
        with pytest.raises(rt_amd.RtHipError) as refused:
            tracer.set_lens(*bad)
        assert refused.value.status == INVALID_ARGUMENT and f"rt_hip_set_lens: {field}" in str(refused.value)
    rgba, _, _ = tracer.render(pod, 64, 36, seed=17, flags=LENS_FLAG)  # (a refused lens left the old one in place)
    assert np.array_equal(rgba, first)
    before = tracer.stats()
    tracer.set_lens(None)
    canvas = np.full((36, 64), 0xDEADBEEF, dtype=np.uint32)
    with pytest.raises(rt_amd.RtHipError) as refused:
        tracer.render(pod, 64, 36, seed=17, flags=LENS_FLAG, out=canvas)
    assert refused.value.status == INVALID_ARGUMENT and "RT_HIP_FLAG_THIN_LENS" in str(refused.value) and "rt_hip_set_lens" in str(refused.value) and (canvas == 0xDEADBEEF).all()
    after = tracer.stats()
    assert (after["segments"], after["kernel"], after["primary_samples"]) == (before["segments"], before["kernel"], before["primary_samples"])


def test_two_ranks_assemble_the_whole_frame(tracer):
    """10a. rt_hip_render_device as ranks 0 and 1 of 2."""
    import torch

    width, height = 96, 54
    pod = camera_pod("basic", "eye", width, height)
    tracer.set_lens(*LENS)
    whole, _, whole_stats = tracer.render(pod, width, height, seed=12, flags=LENS_FLAG)
    tracer.upload(pod)
    padded = rt_amd.padded_local_rows(height, 2, 8)
    gathered = torch.zeros((2, padded, width), dtype=torch.int32, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    segments = 0
    for rank in range(2):
        tracer.render_device(width, height, gathered[rank].data_ptr(), seed=12, flags=LENS_FLAG, partition=(rank, 2, 8), stream=stream)
        torch.cuda.synchronize()
        stats = tracer.stats()
        assert stats["kernel"] == "resident"
        segments += stats["segments"]
        part, _, _ = lens_ref.render(pod, width, height, LENS, seed=12, partition=(rank, 2, 8), want_rgb=False)
        assert np.array_equal(gathered[rank].cpu().numpy().view(np.uint32)[: part.shape[0]], part), rank
    frame = torch.empty((height, width), dtype=torch.int32, device="cuda:0")
    tracer.assemble_device(width, height, 2, 8, gathered.data_ptr(), frame.data_ptr(), stream)
    torch.cuda.synchronize()
    assert np.array_equal(frame.cpu().numpy().view(np.uint32), whole) and segments == whole_stats["segments"]


def test_a_multi_gpu_context_hands_the_lens_to_every_member():
    """10b. rt_hip_create_multi with two members — over two devices where two are visible, else twice the one device (peer copies, as
    tests/test_gpu_multi.py does): the lens set on the context reaches both, and the assembled frame is the whole frame."""
    width, height = 96, 54
    pod = camera_pod("basic", "pinhole", width, height)
    want_rgba, _, want = lens_ref.render(pod, width, height, LENS, seed=19, want_rgb=False)
    two = rt_amd.renderer.device_count() >= 2
    with rt_amd.HipRayTracer(devices=[0, 1] if two else [0, 0], peer_copy=not two) as multi:
        multi.set_lens(*LENS)
        rgba, _, stats = multi.render(pod, width, height, seed=19, flags=LENS_FLAG)
        assert np.array_equal(rgba, want_rgba) and stats["segments"] == want["segments"]
        assert all(multi.member_stats(rank)["kernel"] == "resident" for rank in range(2))


def test_refusals_name_the_flag_and_launch_nothing(tracer):
    """11. Every refusal through the real entry points: the stated status, the flag's name in the message, and afterwards
    rt_hip_stats_fetch still returns the previous frame's counters — nothing was launched."""
    import ctypes as C

    import torch

    pod = camera_pod("basic", "pinhole")
    check_frame(tracer, pod, 64, 36, 1, LENS_FLAG, "resident")
    before = tracer.stats()

    def nothing_ran():
        now = tracer.stats()
        return (now["segments"], now["kernel"], now["primary_samples"]) == (before["segments"], before["kernel"], before["primary_samples"])

    def refused_by_name(call, status=UNSUPPORTED):
        with pytest.raises(rt_amd.RtHipError) as refused:
            call()
        assert refused.value.status == status and "RT_HIP_FLAG_THIN_LENS" in str(refused.value), str(refused.value)
        assert nothing_ran()

    for bit in (capi.RT_HIP_FLAG_FAST, capi.RT_HIP_FLAG_FORCE_TILED, capi.RT_HIP_FLAG_FORCE_RESIDENT, capi.RT_HIP_FLAG_FORCE_STREAMED, capi.RT_HIP_FLAG_FORCE_HALF_CHUNKS, capi.RT_HIP_FLAG_TRACE_BOXES,
                capi.RT_HIP_FLAG_TRACE_BOXES | capi.RT_HIP_FLAG_BOX_BVH, capi.RT_HIP_FLAG_EMISSION, capi.RT_HIP_FLAG_EMISSION | capi.RT_HIP_FLAG_DIRECT_LIGHT):
        canvas = np.full((36, 64), 0xDEADBEEF, dtype=np.uint32)
        refused_by_name(lambda: tracer.render(pod, 64, 36, seed=1, flags=LENS_FLAG | bit, out=canvas))
        assert (canvas == 0xDEADBEEF).all()
    for bit in (12, 15, 20, 30, 31):  # unassigned bits keep their answer
        with pytest.raises(rt_amd.RtHipError) as refused:
            tracer.render(pod, 64, 36, seed=1, flags=LENS_FLAG | (1 << bit))
        assert refused.value.status == UNSUPPORTED and "unknown flag bits" in str(refused.value)
    refused_by_name(lambda: tracer.render_progressive(pod, 64, 36, seed=1, flags=LENS_FLAG))
    refused_by_name(lambda: tracer.render_adaptive(pod, 64, 36, seed=1, flags=LENS_FLAG))
    refused_by_name(lambda: tracer.render_temporal(pod, 64, 36, seed=1, flags=LENS_FLAG))
    refused_by_name(lambda: tracer.render_upscaled(pod, 64, 36, seed=1, flags=LENS_FLAG))
    tracer.upload(pod)
    accum = torch.zeros((36, 64, 3), dtype=torch.float32, device="cuda:0")
    block = torch.zeros((9, 36, 64), dtype=torch.float32, device="cuda:0")
    guide = torch.zeros((36, 64, 8), dtype=torch.float32, device="cuda:0")
    frame = torch.full((36, 64), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    refused_by_name(lambda: tracer.render_pass_device(64, 36, 0, 16, accum.data_ptr(), frame.data_ptr(), flags=LENS_FLAG))
    refused_by_name(lambda: tracer.adaptive_pass_device(64, 36, 0, 16, block.data_ptr(), frame.data_ptr(), flags=LENS_FLAG))
    refused_by_name(lambda: tracer.guide_device(64, 36, guide.data_ptr(), flags=LENS_FLAG))
    # a matrix without a finite eye: a lens needs a perspective matrix — whatever the radius
    flat = camera_pod("basic", "pinhole")
    flat.inverse_view_projection = (C.c_float * 16)(2.4, 0, 0, 0.0, 0, 1.35, 0, 1.0, 0, 0, -12.0, 3.0, 0, 0, 0, 1.0)
    refused_by_name(lambda: tracer.render(flat, 64, 36, seed=1, flags=LENS_FLAG))
    tracer.upload(pod)
    tracer.set_lens(None)
    refused_by_name(lambda: tracer.render_device(64, 36, frame.data_ptr(), flags=LENS_FLAG), INVALID_ARGUMENT)
    torch.cuda.synchronize()
    assert bool((frame == 0x5A5A5A5A).all()) and bool((accum == 0).all()) and bool((block == 0).all()) and bool((guide == 0).all())
    check_frame(tracer, pod, 64, 36, 1, LENS_FLAG, "resident")  # the context renders on
    assert rt_amd.live_frame_locks() == 0


def test_tonemapped_and_bloomed_frames_pass_the_flag_on(tracer):
    """12. rt_hip_render_tonemapped and rt_hip_render_bloomed with the flag: their CPU references applied to the restatement's float frame."""
    pod = camera_pod("dielectric", "eye")
    tracer.set_lens(*LENS)
    _, mean, _ = lens_ref.render(pod, 64, 36, LENS, seed=21)
    p = tonemap_ref.params(curve=tonemap_ref.ACES)
    rgba, rgb, stats, info = tracer.render_tonemapped(pod, 64, 36, seed=21, flags=LENS_FLAG, params=p, want_rgb=True)
    want_rgb, want_rgba, want_state = tonemap_ref.frame(mean, p)
    assert info == tonemap_ref.info_of(want_state) and np.array_equal(rgb.view(np.uint32), want_rgb.view(np.uint32)) and np.array_equal(rgba, want_rgba)
    assert stats["kernel"] == "resident"
    bloom = bloom_ref.params(threshold=0.6)
    rgba, rgb, stats, info = tracer.render_bloomed(pod, 64, 36, seed=21, flags=LENS_FLAG, bloom_params=bloom, tonemap_params=p, want_rgb=True)
    bloomed, _ = bloom_ref.frame(mean, bloom)
    want_rgb, want_rgba, want_state = tonemap_ref.frame(bloomed, p)
    assert info == tonemap_ref.info_of(want_state) and np.array_equal(rgb.view(np.uint32), want_rgb.view(np.uint32)) and np.array_equal(rgba, want_rgba)
    assert not np.array_equal(bloomed.view(np.uint32), mean.view(np.uint32))  # (the glow is not nothing)


def test_render_device_on_a_callers_stream_behind_pending_work():
    """13. One device-level call through tests/stream_harness.py: a non-blocking stream, a sentinel in every output, a delay in front."""
    from tests.stream_harness import Harness, Step, run

    width, height = 37, 23
    pod = camera_pod("basic", "eye", width, height, spp=4)
    want_rgba, want_rgb, _ = lens_ref.render(pod, width, height, LENS, seed=5)
    with rt_amd.HipRayTracer(device=0) as mine:
        mine.set_lens(*LENS)
        mine.upload(pod)
        h = Harness("render_device, thin lens")
        rows = rt_amd.padded_local_rows(height, 1)
        rgba, rgb = h.sink((rows, width)), h.sink((rows, width, 3))
        run([Step(h, lambda: mine.render_device(width, height, rgba.data_ptr(), seed=5, flags=LENS_FLAG, d_rgb_f32=rgb.data_ptr(), stream=h.handle), "lens frame")])
        got_rgba = h.got(rgba).reshape(-1)[: want_rgba.size].reshape(want_rgba.shape)
        got_rgb = h.got(rgb).reshape(-1)[: want_rgb.size].reshape(want_rgb.shape)
        assert np.array_equal(got_rgba, want_rgba) and np.array_equal(got_rgb, want_rgb.view(np.uint32))
