"""RT_HIP_FLAG_BVH_DEVICE_BUILD on the GPU: the hierarchy built by rt_amd/csrc/bvh_build.hip is, byte for byte, the tree of its
serial restatement (tests/native/lbvh_reference.cpp, checked on the CPU by tests/test_bvh_lbvh_reference.py); closest hits
through it are the linear scan's bit for bit; whole frames with the flag equal the frames without it, on every kind of context;
the cached tree remembers its builder; the plug-in's RT_HIP_ACCEL=bvh-device gives RT_HIP_ACCEL=bvh's frame.

The scenes here stop at 5000 spheres, two sort tiles and one trip of the scan.  tests/test_gpu_bvh_device_build_scale.py goes on
from there: every edge of the sort and of the per-sphere kernels up to 262145 spheres, the large sort and the always list over
several tiles, closest hits and frames through trees of 100000."""
import os
import subprocess

import numpy as np
import pytest

import rt_amd
from rt_amd import capi
from tests import bvh_cases, lbvh_cases
from tests.bvh_cases import MATERIALS, adversarial_rays, sphere_field, sphere_scene

pytestmark = pytest.mark.gpu

BVH = capi.RT_HIP_FLAG_BVH
DEVICE = capi.RT_HIP_FLAG_BVH | getattr(capi, "RT_HIP_FLAG_BVH_DEVICE_BUILD", 1 << 11)
SM = capi.RT_HIP_FLAG_SM_MATERIALS
ROOT = __import__("pathlib").Path(__file__).resolve().parent.parent


# ---- the tree's bytes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", lbvh_cases.scene_names())
def test_the_device_tree_is_the_serial_restatements(tracer, name):
    for rows in lbvh_cases.scenes_of(name):
        scene = sphere_scene(rows)
        tracer.upload(scene)
        got = tracer.kat_bvh_build_device()
        bvh_cases.check_tree(scene, got)
        want = lbvh_cases.reference_tree(scene)
        assert [int(c) for c in want["counts"]] == [len(got["nodes"]), len(got["order"]), len(got["always"]), got["depth"], got["root"]]
        same, where = lbvh_cases.same_bytes(got, want)
        assert same, f"{name}: the device tree's {where} differ from the serial restatement's"
        again = tracer.kat_bvh_build_device()
        same, where = lbvh_cases.same_bytes(got, again)
        assert same, f"{name}: two builds differ in {where}"


# ---- closest hits ---------------------------------------------------------------------------------------------------------
def same_hits(tracer, pod, origins, dirs, what):
    tracer.upload(pod)
    linear = tracer.kat_closest_hit(origins, dirs)
    tree = tracer.kat_closest_hit(origins, dirs, device_build=True)
    for g, l, label in zip(tree, linear, ("distance", "kind", "index", "normal")):
        bad = np.nonzero((g.view(np.uint32) != l.view(np.uint32)).reshape(len(origins), -1).any(axis=1))[0]
        assert len(bad) == 0, f"{what}: {label} through the device tree differs from the linear scan for {len(bad)} rays, first {bad[0]}: o={origins[bad[0]]} d={dirs[bad[0]]} tree={g[bad[0]]} linear={l[bad[0]]}"
    return linear


@pytest.mark.parametrize("count,seed", [(300, 1), (5000, 3)])
def test_closest_hit_on_adversarial_rays(tracer, count, seed):
    rng = np.random.default_rng(seed)
    spheres = sphere_field(rng, count)
    for j in range(20):  # duplicates far apart in the index order, and nested spheres
        spheres.append(spheres[1 + j * 7])
        x, y, z, r, m = spheres[2 + j * 11]
        spheres.append((x, y, z, r * 0.5, m))
    pod = rt_amd.scene_from_arrays(spheres, [(0, 1, 0, 0.5, 2)] if seed % 2 else [], MATERIALS)
    origins, dirs = adversarial_rays(spheres, rng)
    linear = same_hits(tracer, pod, origins, dirs, f"{count} spheres")
    assert (linear[1] == 1).mean() > 0.3


@pytest.mark.parametrize("name", list(bvh_cases.REGIMES))
def test_closest_hit_in_every_regime_of_the_cull_bound(tracer, name):
    for label, rows, origins, dirs in lbvh_cases.regime(name):
        same_hits(tracer, sphere_scene(rows), origins, dirs, f"{name} / {label}")


def rays_at(rows, targets, rng, count):
    c, r = bvh_cases.rounded(rows)
    pick = rng.choice(targets, size=count)
    d = bvh_cases.unit(rng.normal(size=(count, 3)))
    aim = c[pick] + rng.uniform(-0.5, 0.5, (count, 3)) * r[pick, None]
    return (aim - d * rng.uniform(30, 60, (count, 1))).astype(np.float32), bvh_cases.normalised(d)


@pytest.mark.parametrize("which", ["identical", "distinct"])
def test_closest_hit_with_an_always_list_at_its_cap(tracer, which):
    made = bvh_cases.always_cap_identical() if which == "identical" else bvh_cases.always_cap_distinct()
    rows, large = made[0], made[1]
    rng = np.random.default_rng(51)
    outside_o, outside_d = rays_at(rows, large, rng, 4000)
    near_o, near_d = bvh_cases.near_rays(rows, rng, 4000, 1.0)
    dist, kind, index, _ = same_hits(tracer, sphere_scene(rows), np.concatenate([outside_o, near_o]), np.concatenate([outside_d, near_d]), f"always list, {which}")
    assert (kind[:4000] == 1).all()


def test_closest_hit_through_a_tree_as_deep_as_the_stack(tracer):
    rows = lbvh_cases.morton_staircase()
    rng = np.random.default_rng(53)
    origins, dirs = bvh_cases.near_rays(rows, rng, 20000, 1.0)
    pod = sphere_scene(rows)
    same_hits(tracer, pod, origins, dirs, "morton staircase")
    assert tracer.kat_bvh_build_device()["depth"] == bvh_cases.STACK_DEPTH


# ---- frames ---------------------------------------------------------------------------------------------------------------
def field_pod(count, seed, width, height, spp, planes=0):
    rng = np.random.default_rng(seed)
    spheres = sphere_field(rng, count)
    plane_rows = [(0, 1, 0, 0.05 * (k + 1), k % len(MATERIALS)) for k in range(planes)]
    camera = rt_amd.Scene.parse("").set_camera((0.0, 4.0, 3.0), (0.0, -0.35, -1.0))
    ivp = camera.describe(width, height).inverse_view_projection[:]
    return rt_amd.scene_from_arrays(spheres, plane_rows, MATERIALS, samples_per_pixel=spp, max_bounces=7, inverse_view_projection=ivp)


def same_frame(got, want, what):
    (got_rgba, got_rgb, got_stats), (want_rgba, want_rgb, want_stats) = got, want
    same = (got_rgb.view(np.uint32) == want_rgb.view(np.uint32)) | (np.isnan(got_rgb) & np.isnan(want_rgb))
    assert same.all(), f"{what}: float mean differs in {(~same).any(axis=-1).sum()} pixels"
    assert np.array_equal(got_rgba, want_rgba), f"{what}: packed pixels differ"
    assert got_stats["segments"] == want_stats["segments"], what


@pytest.mark.parametrize("count,planes", [(1, 0), (5, 0), (9, 1), (64, 2), (700, 0), (5000, 1)])
@pytest.mark.parametrize("flags", [0, SM], ids=["mg", "sm"])
def test_frames_equal_the_linear_frames(tracer, count, planes, flags):
    width, height, spp = 64, 48, 4
    pod = field_pod(count, 60 + count, width, height, spp, planes)
    want = tracer.render(pod, width, height, seed=count, flags=flags, want_rgb=True)
    got = tracer.render(pod, width, height, seed=count, flags=flags | DEVICE, want_rgb=True)
    assert got[2]["kernel"] == "bvh"
    same_frame(got, want, f"{count} spheres, {planes} planes")


def test_frame_of_the_cluster_chain(tracer):
    width, height, spp = 64, 48, 4
    rows = bvh_cases.cluster_chain(0, 1.0)
    rows[:, 4] = np.arange(len(rows)) % len(MATERIALS)
    camera = rt_amd.Scene.parse("").set_camera((-1.0, 0.0, 0.0), (1.0, 0.0, 0.0))
    ivp = camera.describe(width, height).inverse_view_projection[:]
    pod = rt_amd.scene_from_arrays(rows, [(0, 1, 0, 0.5, 1), (0.6, 0.8, 0, 2.0, 2)], MATERIALS, samples_per_pixel=spp, max_bounces=6, inverse_view_projection=ivp)
    want = tracer.render(pod, width, height, seed=12, want_rgb=True)
    got = tracer.render(pod, width, height, seed=12, flags=DEVICE, want_rgb=True)
    assert got[2]["kernel"] == "bvh"
    same_frame(got, want, "cluster chain")


def test_a_partition_share(tracer):
    import torch

    width, height, spp, part = 64, 48, 4, (1, 3, 8)
    pod = field_pod(700, 71, width, height, spp, 1)
    tracer.upload(pod)
    rows = rt_amd.renderer.local_rows(height, *part)
    frames = []
    for flags in (0, DEVICE):
        frame = torch.zeros((rows, width), dtype=torch.int32, device="cuda:0")
        tracer.render_device(width, height, frame.data_ptr(), seed=9, flags=flags, partition=part, stream=torch.cuda.current_stream().cuda_stream)
        stats = tracer.stats()
        frames.append((frame.cpu().numpy().view(np.uint32), stats["segments"], stats["kernel"]))
    assert frames[1][2] == "bvh"
    assert np.array_equal(frames[0][0], frames[1][0]) and frames[0][1] == frames[1][1]
    assert len(np.unique(frames[0][0])) > 50


def test_multi_member_context(tracer):
    width, height, spp = 64, 48, 4
    pod = field_pod(1500, 21, width, height, spp)
    want, _, _ = tracer.render(pod, width, height, seed=4)
    with rt_amd.HipRayTracer(devices=[0, 0], peer_copy=True) as multi:
        got, _, _ = multi.render(pod, width, height, seed=4, flags=DEVICE)
        again, _, _ = multi.render(pod, width, height, seed=4, flags=DEVICE)
    assert np.array_equal(got, want) and np.array_equal(again, want)


# ---- the cache ------------------------------------------------------------------------------------------------------------
def test_the_cached_tree_remembers_its_builder(tracer):
    width, height, spp = 64, 48, 4
    rng = np.random.default_rng(11)
    spheres = sphere_field(rng, 1200)
    camera = rt_amd.Scene.parse("").set_camera((0.0, 4.0, 3.0), (0.0, -0.35, -1.0))
    ivp = camera.describe(width, height).inverse_view_projection[:]
    first = rt_amd.scene_from_arrays(spheres, [], MATERIALS, samples_per_pixel=spp, max_bounces=5, inverse_view_projection=ivp)
    frames = [tracer.render(first, width, height, seed=3, flags=flags, want_rgb=True) for flags in (0, BVH, DEVICE, BVH)]
    assert [f[2]["kernel"] for f in frames[1:]] == ["bvh"] * 3
    for k, frame in enumerate(frames[1:]):
        same_frame(frame, frames[0], f"frame {k + 1} of linear, host tree, device tree, host tree")
    moved = list(spheres)
    moved[1] = (0.0, 1.5, -6.0, 1.2, 1)  # same count, one sphere moved (and grown) into view
    second = rt_amd.scene_from_arrays(moved, [], MATERIALS, samples_per_pixel=spp, max_bounces=5, inverse_view_projection=ivp)
    got = tracer.render(second, width, height, seed=3, flags=DEVICE, want_rgb=True)
    want = tracer.render(second, width, height, seed=3, want_rgb=True)
    assert got[2]["kernel"] == "bvh"
    same_frame(got, want, "after the move")
    assert not np.array_equal(want[0], frames[0][0])  # the move is visible


# ---- refusals, the preview, the plug-in -------------------------------------------------------------------------------------
def test_refusals_and_the_preview(tracer):
    pod = field_pod(300, 8, 32, 18, 2)
    alone = DEVICE & ~BVH
    refused_flags = [alone] + [DEVICE | force for force in (capi.RT_HIP_FLAG_FORCE_TILED, capi.RT_HIP_FLAG_FORCE_RESIDENT, capi.RT_HIP_FLAG_FORCE_STREAMED, capi.RT_HIP_FLAG_FAST)]
    refused_flags += [alone | force for force in (capi.RT_HIP_FLAG_FORCE_TILED, capi.RT_HIP_FLAG_FORCE_RESIDENT, capi.RT_HIP_FLAG_FORCE_STREAMED, capi.RT_HIP_FLAG_FAST)]
    for flags in refused_flags:
        with pytest.raises(capi.RtHipError) as refused:
            tracer.render(pod, 32, 18, seed=1, flags=flags)
        assert refused.value.status == 5, hex(flags)  # RT_HIP_UNSUPPORTED
    preview, _, stats = tracer.render(pod, 32, 18, flags=capi.RT_HIP_FLAG_PREVIEW | DEVICE)
    assert stats["kernel"] == "preview"
    want, _, _ = tracer.render(pod, 32, 18, flags=capi.RT_HIP_FLAG_PREVIEW)
    assert np.array_equal(preview, want)
    good, _, stats = tracer.render(pod, 32, 18, seed=1, flags=DEVICE)  # and the flag itself is taken
    assert stats["kernel"] == "bvh"


def test_plugin_accel_bvh_device(tmp_path):
    rng = np.random.default_rng(17)
    rows = ["    { material = 0, position = [0, -1000, 0], radius = 1000 },"]
    for _ in range(1999):
        r = rng.uniform(0.05, 0.3)
        rows.append(f"    {{ material = {int(rng.integers(1, 3))}, position = [{rng.uniform(-12, 12):.4f}, {r:.4f}, {rng.uniform(-24, 0):.4f}], radius = {r:.4f} }},")
    text = "camera = { position = [0, 4, 3], direction = [0, -0.35, -1] }\n"
    text += "materials = [\n    { type = 'lambert', albedo = [0.5, 0.5, 0.5] },\n    { type = 'lambert', albedo = [0.9, 0.3, 0.2] },\n    { type = 'metal', albedo = [0.9, 0.9, 0.9], roughness = 0.1 },\n]\n"
    text += "spheres = [\n" + "\n".join(rows) + "\n]\n"
    scene = tmp_path / "field.toml"
    scene.write_text(text)
    binary = ROOT / "rt_amd" / "bin" / "rt_headless"
    outs = []
    for accel in ("bvh", "bvh-device"):
        out = tmp_path / f"frame_{accel}.ppm"
        env = dict(os.environ, RT_HIP_SEED="5", RT_HIP_ACCEL=accel)
        done = subprocess.run([str(binary), "--renderer", "hip", "--scene", str(scene), "--size", "80x45", "--spp", "4", "--frames", "1", "--out", str(out)], env=env, capture_output=True, text=True, timeout=300)
        assert done.returncode == 0 and "error" not in done.stderr, done.stderr
        outs.append(out.read_bytes())
    assert outs[0] == outs[1]
    assert len(set(outs[0][-3000:])) > 4  # the field is in the picture
