"""RT_HIP_FLAG_DIRECT_LIGHT on the GPU: every frame is compared bit for bit — packed pixels, float mean, segments — with
the CPU restatement (tests/native/direct_reference.cpp: light_reference.cpp's loop plus the vertex rule of
rt_amd/csrc/direct_light_rules.hpp), and the kernel that ran is checked.  Tolerance 0 everywhere.  The cases walk the eight direct
builds — the resident kernel's LDS scan through a pinhole and a tilted camera, its scalar-load scan, the hierarchy kernel with both
builders, each with the mg and the sm table — and the rule's branches: the cap of 256, the inside branch, a plane light beside a
sphere light, a partition, no sampled light at all.

No test here compares the flag's frame with the RT_HIP_FLAG_EMISSION frame's mean: the two converge to different images (§3.13)."""
import numpy as np
import pytest

import rt_amd
from oracle import binding as oracle
from rt_amd import capi
from tests import direct_reference as direct_ref
from tests import light_reference as light_ref

pytestmark = pytest.mark.gpu

EMISSION = capi.RT_HIP_FLAG_EMISSION
DIRECT = capi.RT_HIP_FLAG_EMISSION | capi.RT_HIP_FLAG_DIRECT_LIGHT
SM = capi.RT_HIP_FLAG_SM_MATERIALS
INVALID_ARGUMENT, UNSUPPORTED = 1, 5
PINHOLE = ((0.3, 1.5, 5.0), (0, 0, -1))
TILTED = ((0.3, 1.5, 5.0), (0.2, -0.15, -1))


@pytest.fixture(autouse=True)
def _no_table_outlives_a_test(tracer):
    yield
    tracer.set_emission(None)  # (the session's context is shared: no other test file sees a table)


def check_frame(tracer, pod, width, height, seed, flags, kernel, table):
    """rt_hip_render with `flags` under `table` against direct_ref_render: rgba8, rgb_f32, segments; kernel_variant."""
    tracer.set_emission(table)
    rgba, rgb, stats = tracer.render(pod, width, height, seed=seed, flags=flags, want_rgb=True)
    want_rgba, want_rgb, want = direct_ref.render(pod, width, height, table, seed=seed, sm_materials=bool(flags & SM), direct=bool(flags & capi.RT_HIP_FLAG_DIRECT_LIGHT))
    assert stats["kernel"] == kernel, stats
    assert np.array_equal(rgba, want_rgba), f"{(rgba != want_rgba).sum()} of {rgba.size} pixels differ from the restatement's"
    assert np.array_equal(rgb.view(np.uint32), want_rgb.view(np.uint32))
    assert stats["segments"] == want["segments"]
    return rgba, rgb, stats


@pytest.mark.parametrize("table", [0, SM])
@pytest.mark.parametrize("camera,form", [(PINHOLE, "pinhole"), (TILTED, "eye")])
def test_lights_toml(tracer, table, camera, form):
    """The scene of the flag at 96x54, both tables, an axis-aligned and a tilted camera: the four LDS-scan builds.  The shadow queries are
    segments: the frame counts more of them than the RT_HIP_FLAG_EMISSION frame does."""
    pod = light_ref.lights_scene(*camera).describe(96, 54)
    assert oracle.primary_ray(pod, 96, 54, 0, 0, want_form=True)[2] == form
    _, _, stats = check_frame(tracer, pod, 96, 54, 11, DIRECT | table, "resident", light_ref.LIGHTS_TABLE)
    _, _, implicit = light_ref.render(pod, 96, 54, light_ref.LIGHTS_TABLE, seed=11, want_rgb=False, sm_materials=bool(table))
    assert stats["segments"] > implicit["segments"]


@pytest.mark.parametrize("spp", [16, 17, 48])
def test_chunk_counts(tracer, spp):
    """One chunk, a chunk and a tail of one, three chunks."""
    pod = light_ref.lights_scene(spp=spp).describe(96, 54)
    check_frame(tracer, pod, 96, 54, 14, DIRECT, "resident", light_ref.LIGHTS_TABLE)


@pytest.mark.parametrize("bounces", [1, 2, 50])
def test_bounce_counts(tracer, bounces):
    """max_bounces 1 is "primary hit plus direct light": a shadow segment consumes no bounce; 50 lets paths run long past one step per vertex."""
    pod = light_ref.lights_scene(bounces=bounces).describe(96, 54)
    for sm in (0, SM):
        _, rgb, _ = check_frame(tracer, pod, 96, 54, 15, DIRECT | sm, "resident", light_ref.LIGHTS_TABLE)
    if bounces == 1:
        assert (rgb > 0).any()  # (the last table's frame: direct light reaches surfaces although no path may bounce)


@pytest.fixture(scope="module")
def camera():
    return rt_amd.Scene.named("basic").describe(64, 36)


def one_light(n_materials=4, rgb=(2.0, 1.5, 1.0), which=3):
    table = np.zeros((n_materials, 3), dtype=np.float32)
    table[which] = rgb
    return table


def field(lights_every=16):
    """48 spheres (the scalar-load scan starts at 40) of which every sixteenth — 3 — is a light: material 3 glows, the others cycle 0..2"""
    spheres = [(x, y, z, r, 3 if i % lights_every == 5 else i % 3) for i, (x, y, z, r, _) in enumerate(light_ref.grid_spheres(48))]
    assert sum(1 for s in spheres if s[4] == 3) == 3
    return spheres


def test_the_scalar_load_build(tracer, camera):
    pod = light_ref.scene_pod(camera, spheres=field(), planes=[(0, 1, 0, 0, 0)], spp=16)
    assert direct_ref.count(pod, one_light()) == 3
    for table in (0, SM):
        check_frame(tracer, pod, 64, 36, 5, DIRECT | table, "resident", one_light())


@pytest.mark.parametrize("build", [0, capi.RT_HIP_FLAG_BVH_DEVICE_BUILD])
def test_the_hierarchy_build(tracer, camera, build):
    """The same field under RT_HIP_FLAG_BVH, the host's tree and the device builder's."""
    pod = light_ref.scene_pod(camera, spheres=field(), planes=[(0, 1, 0, 0, 0)], spp=16)
    for table in (0, SM):
        check_frame(tracer, pod, 64, 36, 6, DIRECT | capi.RT_HIP_FLAG_BVH | build | table, "bvh", one_light())


def test_the_cap(tracer):
    """300 spheres of which 260 are lights: the first 256 are sampled, the other 4 count on hit."""
    camera = rt_amd.Scene.named("basic").describe(32, 18)
    spheres = [(x, y, z, r, 0 if i % 15 in (3, 9) else 3) for i, (x, y, z, r, _) in enumerate(light_ref.grid_spheres(300, radius=0.1, pitch=0.25))]
    assert sum(1 for s in spheres if s[4] == 3) == 260
    pod = light_ref.scene_pod(camera, spheres=spheres, planes=[(0, 1, 0, 0, 0)], spp=16)
    table = one_light(rgb=(0.5, 0.4, 0.3))
    assert direct_ref.count(pod, table) == direct_ref.MAX_SAMPLED_LIGHTS
    check_frame(tracer, pod, 32, 18, 7, DIRECT, "resident", table)
    check_frame(tracer, pod, 32, 18, 7, DIRECT | capi.RT_HIP_FLAG_BVH, "bvh", table)


def test_inside_an_emitting_sphere(tracer):
    """A lambert sphere and the camera inside an emitting sphere: the inside branch samples the whole sphere, no flip."""
    width, height = 64, 36
    camera = rt_amd.Scene.named("basic").describe(width, height)  # (its eye at (0, 1, 3))
    pod = light_ref.scene_pod(camera, spheres=[(0, 1, 3, 50, 1), (0, 1, 0, 0.8, 0), (1.5, 0.6, 0.5, 0.4, 3)], spp=16, bounces=4)
    for sm in (0, SM):
        _, rgb, _ = check_frame(tracer, pod, width, height, 3, DIRECT | sm, "resident", one_light(which=1, rgb=(0.5, 0.5, 0.5)))
    assert (rgb > 0).all()


def test_a_plane_light_beside_a_sphere_light(tracer, camera):
    """The ceiling counts on hit, the lamp is sampled; a degenerate light sphere (radius 0) counts on hit too."""
    pod = light_ref.scene_pod(camera, spheres=[(0, 0.5, 0, 0.5, 3), (1.2, 1.5, 0.2, 0.25, 1), (-1, 0.4, 0.5, 0.0, 1)], planes=[(0, 1, 0, 0, 0), (0, 1, 0, -4, 1)], spp=16)
    table = one_light(which=1, rgb=(1.5, 1.5, 1.25))
    assert direct_ref.count(pod, table) == 1
    check_frame(tracer, pod, 64, 36, 12, DIRECT, "resident", table)


def test_rank_1_of_3_renders_its_rows_of_the_whole_frame(tracer):
    import torch

    width, height = 96, 54
    pod = light_ref.lights_scene().describe(width, height)
    whole, _, _ = direct_ref.render(pod, width, height, light_ref.LIGHTS_TABLE, seed=12, want_rgb=False)
    tracer.set_emission(light_ref.LIGHTS_TABLE)
    tracer.upload(pod)
    padded = rt_amd.padded_local_rows(height, 3, 8)
    rows = torch.zeros((padded, width), dtype=torch.int32, device="cuda:0")
    tracer.render_device(width, height, rows.data_ptr(), seed=12, flags=DIRECT, partition=(1, 3, 8), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    stats = tracer.stats()
    mine = [y for y in range(height) if (y // 8) % 3 == 1]
    part, _, want = direct_ref.render(pod, width, height, light_ref.LIGHTS_TABLE, seed=12, partition=(1, 3, 8), want_rgb=False)
    got = rows.cpu().numpy().view(np.uint32)[: len(mine)]
    assert np.array_equal(got, part) and np.array_equal(got, whole[mine])
    assert stats["kernel"] == "resident" and stats["segments"] == want["segments"]


def test_without_a_light_sphere_the_frame_is_the_emission_frame(tracer, camera):
    """Only a plane glows: no sampled light — frame, float mean, segments and kernel_variant of RT_HIP_FLAG_EMISSION alone."""
    pod = light_ref.scene_pod(camera, spheres=[(0, 0.5, 0, 0.5, 3), (1, 0.5, 0.5, 0.5, 0)], planes=[(0, 1, 0, 0, 0), (0, 1, 0, -4, 1)])
    table = one_light(which=1)
    assert direct_ref.count(pod, table) == 0
    tracer.set_emission(table)
    implicit = tracer.render(pod, 64, 36, seed=9, flags=EMISSION, want_rgb=True)
    flagged = tracer.render(pod, 64, 36, seed=9, flags=DIRECT, want_rgb=True)
    assert np.array_equal(implicit[0], flagged[0]) and np.array_equal(implicit[1].view(np.uint32), flagged[1].view(np.uint32))
    assert (implicit[2]["kernel"], implicit[2]["segments"]) == (flagged[2]["kernel"], flagged[2]["segments"])
    want_rgba, _, want = light_ref.render(pod, 64, 36, table, seed=9, want_rgb=False)
    assert np.array_equal(flagged[0], want_rgba) and flagged[2]["segments"] == want["segments"]


def test_the_list_follows_the_table_and_the_scene(tracer, camera):
    """The list is built with the light variant of the tables: a new table, then a new scene, and frames of RT_HIP_FLAG_EMISSION alone in
    between keep their own answer."""
    pod = light_ref.lights_scene().describe(64, 36)
    first, _, _ = check_frame(tracer, pod, 64, 36, 17, DIRECT, "resident", light_ref.LIGHTS_TABLE)
    check_frame(tracer, pod, 64, 36, 17, EMISSION, "resident", light_ref.LIGHTS_TABLE)
    other = np.zeros((5, 3), dtype=np.float32)
    other[2] = (0.5, 2, 0.5)  # the clay sphere glows instead
    second, _, _ = check_frame(tracer, pod, 64, 36, 17, DIRECT, "resident", other)
    assert (first != second).mean() > 0.05
    four = light_ref.scene_pod(camera, spheres=[(0, 0.5, 0, 0.5, 1), (1, 0.5, 0.5, 0.5, 0)], planes=[(0, 1, 0, 0, 0)])
    check_frame(tracer, four, 64, 36, 17, DIRECT, "resident", one_light(which=1))
    again, _, _ = check_frame(tracer, pod, 64, 36, 17, DIRECT, "resident", light_ref.LIGHTS_TABLE)
    assert np.array_equal(first, again)


def test_a_multi_gpu_context_builds_the_list_on_every_member(camera):
    """rt_hip_create_multi with two members — over two devices where two are visible, else twice the one device (peer copies, as
    tests/test_gpu_lights.py does): the sampled-light list is built per member (§3.13), so the assembled frame is the restatement's whole
    frame and both members ran the resident kernel; and it FOLLOWS the table and the scene on every member — another table, then a scene
    with another sphere count, each frame again the restatement's."""
    width, height = 96, 54
    pod = light_ref.lights_scene().describe(width, height)
    other = np.zeros((5, 3), dtype=np.float32)
    other[2] = (0.5, 2, 0.5)  # the clay sphere glows instead
    wide = rt_amd.Scene.named("basic").describe(width, height)
    two_spheres = light_ref.scene_pod(wide, spheres=[(0, 0.5, 0, 0.5, 1), (1, 0.5, 0.5, 0.5, 0)], planes=[(0, 1, 0, 0, 0)])
    assert two_spheres.n_spheres != pod.n_spheres and direct_ref.count(pod, other) == 1 and direct_ref.count(two_spheres, one_light(which=1)) == 1
    two = rt_amd.renderer.device_count() >= 2
    with rt_amd.HipRayTracer(devices=[0, 1] if two else [0, 0], peer_copy=not two) as multi:
        frames = []
        for scene, table in ((pod, light_ref.LIGHTS_TABLE), (pod, other), (two_spheres, one_light(which=1)), (pod, light_ref.LIGHTS_TABLE)):
            want_rgba, _, want = direct_ref.render(scene, width, height, table, seed=19, want_rgb=False)
            multi.set_emission(table)
            rgba, _, stats = multi.render(scene, width, height, seed=19, flags=DIRECT)
            assert np.array_equal(rgba, want_rgba), f"{(rgba != want_rgba).sum()} of {rgba.size} pixels differ from the restatement's"
            assert stats["segments"] == want["segments"]
            assert all(multi.member_stats(rank)["kernel"] == "resident" for rank in range(2))
            frames.append(rgba)
        assert (frames[0] != frames[1]).mean() > 0.05 and np.array_equal(frames[0], frames[3])


def test_refusals_name_the_flag_and_launch_nothing(tracer):
    import torch

    pod = light_ref.lights_scene().describe(64, 36)
    check_frame(tracer, pod, 64, 36, 1, DIRECT, "resident", light_ref.LIGHTS_TABLE)
    before = tracer.stats()
    ALONE = capi.RT_HIP_FLAG_DIRECT_LIGHT

    def refused_by_name(call, status=UNSUPPORTED, name="RT_HIP_FLAG_DIRECT_LIGHT"):
        with pytest.raises(rt_amd.RtHipError) as refused:
            call()
        assert refused.value.status == status and name in str(refused.value), str(refused.value)
        now = tracer.stats()
        assert (now["segments"], now["kernel"], now["primary_samples"]) == (before["segments"], before["kernel"], before["primary_samples"])

    canvas = np.full((36, 64), 0xDEADBEEF, dtype=np.uint32)
    refused_by_name(lambda: tracer.render(pod, 64, 36, seed=1, flags=ALONE, out=canvas))  # not without RT_HIP_FLAG_EMISSION
    for bit in (capi.RT_HIP_FLAG_FAST, capi.RT_HIP_FLAG_FORCE_TILED, capi.RT_HIP_FLAG_FORCE_RESIDENT, capi.RT_HIP_FLAG_FORCE_STREAMED, capi.RT_HIP_FLAG_FORCE_HALF_CHUNKS, capi.RT_HIP_FLAG_TRACE_BOXES,
                capi.RT_HIP_FLAG_TRACE_BOXES | capi.RT_HIP_FLAG_BOX_BVH):
        refused_by_name(lambda: tracer.render(pod, 64, 36, seed=1, flags=DIRECT | bit, out=canvas))
    assert (canvas == 0xDEADBEEF).all()
    for bit in (12, 15, 20, 31):  # unassigned bits keep their answer
        with pytest.raises(rt_amd.RtHipError) as refused:
            tracer.render(pod, 64, 36, seed=1, flags=DIRECT | (1 << bit))
        assert refused.value.status == UNSUPPORTED and "unknown flag bits" in str(refused.value)
    refused_by_name(lambda: tracer.render_progressive(pod, 64, 36, seed=1, flags=ALONE))
    refused_by_name(lambda: tracer.render_adaptive(pod, 64, 36, seed=1, flags=ALONE))
    refused_by_name(lambda: tracer.render_temporal(pod, 64, 36, seed=1, flags=ALONE))
    refused_by_name(lambda: tracer.render_progressive(pod, 64, 36, seed=1, flags=DIRECT), name="RT_HIP_FLAG_EMISSION")  # (the flag it modifies is named first)
    tracer.upload(pod)
    guide = torch.zeros((36, 64, 8), dtype=torch.float32, device="cuda:0")
    refused_by_name(lambda: tracer.guide_device(64, 36, guide.data_ptr(), flags=ALONE))
    tracer.set_emission(None)
    frame = torch.full((36, 64), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    refused_by_name(lambda: tracer.render_device(64, 36, frame.data_ptr(), flags=DIRECT), INVALID_ARGUMENT, name="RT_HIP_FLAG_EMISSION")  # no table
    torch.cuda.synchronize()
    assert bool((frame == 0x5A5A5A5A).all()) and bool((guide == 0).all())
    check_frame(tracer, pod, 64, 36, 1, DIRECT, "resident", light_ref.LIGHTS_TABLE)  # the context renders on
    # the preview ignores the flag
    plain, _, _ = tracer.render(pod, 64, 36, seed=1, flags=capi.RT_HIP_FLAG_PREVIEW)
    flagged, _, _ = tracer.render(pod, 64, 36, seed=1, flags=capi.RT_HIP_FLAG_PREVIEW | DIRECT)
    assert np.array_equal(plain, flagged)
    assert rt_amd.live_frame_locks() == 0


def test_the_rules_header_on_the_device_is_the_header_g_plus_plus_compiles(tracer):
    """The two known-answer entries (include/rt_hip_kat.h): the octahedral map and the aim with its weight, bit for bit — corners, fold
    lines, random numerators; vertices outside and inside the light, facing it and facing away, on top of its centre."""
    top, half = (1 << 24) - 1, 1 << 23
    rng = np.random.default_rng(17)
    special = [0, 1, half - 1, half, half + 1, half // 2, half + half // 2, top - 1, top]
    ka = np.array([a for a in special for _ in special] + list(rng.integers(0, 1 << 24, 400)), dtype=np.uint32)
    kb = np.array([b for _ in special for b in special] + list(rng.integers(0, 1 << 24, 400)), dtype=np.uint32)
    got = tracer.kat_direct_octahedral(ka, kb)
    want = np.array([direct_ref.octahedral(int(a), int(b)) for a, b in zip(ka, kb)], dtype=np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))

    n = ka.size
    x = rng.uniform(-3, 3, (n, 3)).astype(np.float32)
    normal = rng.normal(size=(n, 3))
    normal = (normal / np.linalg.norm(normal, axis=1, keepdims=True)).astype(np.float32)
    centre = rng.uniform(-3, 3, (n, 3)).astype(np.float32)
    radius = rng.uniform(0.05, 4.0, n).astype(np.float32)  # (a third of the vertices end up inside their light)
    centre[:5] = x[:5]  # the vertex on top of the centre
    radius[5:10] = np.float32(1e-30)  # R * R underflows: the weight is 0 or not finite, the rule must say the same thing on both sides
    vectors = np.concatenate([x, normal, centre], axis=1)
    for n_lights in (1, 3, 256):
        got = tracer.kat_direct_aim(ka, kb, vectors, radius, n_lights)
        want = np.array([direct_ref.aim(int(a), int(b), x[i], normal[i], centre[i], radius[i], n_lights) for i, (a, b) in enumerate(zip(ka, kb))], dtype=np.float32)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1))[:8]
        inside = ((x - centre) ** 2).sum(axis=1) < radius * radius
        assert 50 < (want[:, 4] == 1).sum() < n and inside.sum() > 50 and (want[inside, 4] == 1).sum() > 10 and (want[~inside, 4] == 1).sum() > 10
