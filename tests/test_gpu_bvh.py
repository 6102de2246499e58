"""RT_HIP_FLAG_BVH on the GPU: the spheres through the bounding volume hierarchy give the linear scan's answer, bit for bit.

The closest-hit entry of the test-only library runs the render kernel's own traversal (bvh_scan.hpp) on rays chosen to sit on
the cull bound's edge — tangents a few ulp off, origins on and inside spheres, duplicates in different leaves — against the
linear scan and the oracle; whole frames with the flag equal the frames without it (and the oracle's), on every context kind."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import rt_amd
from oracle import binding as oracle
from rt_amd import capi
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu

BVH = capi.RT_HIP_FLAG_BVH
SM = capi.RT_HIP_FLAG_SM_MATERIALS
ROOT = __import__("pathlib").Path(__file__).resolve().parent.parent
MATERIALS = [(0, 1, 1, 1, 1, 0.5, 0.5), (1, 0.9, 0.9, 0.9, 1, 0.1, 0.8), (0, 0.3, 0.6, 0.9, 1, 0.5, 0.5), (2, 1, 1, 1, 1, 0.0, 1.5), (1, 0.8, 0.6, 0.2, 1, 0.4, 0.8)]


def normalised(v):
    v = np.asarray(v, dtype=np.float64).reshape(-1, 3)
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def same_hits(tracer, pod, origins, dirs, what):
    tracer.upload(pod)
    linear = tracer.kat_closest_hit(origins, dirs)
    tree = tracer.kat_closest_hit(origins, dirs, bvh=True)
    want = oracle.closest_hit(pod, origins, dirs)
    finite = np.isfinite(dirs).all(axis=1)
    for g, l, w, label in zip(tree, linear, want, ("distance", "kind", "index", "normal")):
        assert np.array_equal(l[finite].view(np.uint32), w[finite].view(np.uint32)), f"{what}: linear scan {label} is not the oracle's"
        bad = np.nonzero((g.view(np.uint32) != l.view(np.uint32)).reshape(len(origins), -1).any(axis=1))[0]
        assert len(bad) == 0, f"{what}: BVH {label} differs from the linear scan for {len(bad)} rays, first {bad[0]}: o={origins[bad[0]]} d={dirs[bad[0]]} bvh={g[bad[0]]} linear={l[bad[0]]}"
    return linear


def sphere_field(rng, count, spread=12.0):
    spheres = [(0.0, -1000.0, 0.0, 1000.0, 0)]
    for _ in range(count - 1):
        r = rng.uniform(0.05, 0.3)
        spheres.append((rng.uniform(-spread, spread), r, rng.uniform(-2 * spread, 0), r, int(rng.integers(1, len(MATERIALS)))))
    return spheres


def adversarial_rays(spheres, rng, per_sphere=8):
    """Tangent and near-tangent rays (offsets of +-1..64 ulp of r from the tangent line), origins on and inside spheres."""
    origins, dirs = [], []
    s = np.asarray(spheres, dtype=np.float64)
    picks = rng.choice(len(s), size=min(len(s), 400), replace=False)
    for i in picks:
        c, r = s[i, :3].astype(np.float32).astype(np.float64), abs(float(np.float32(s[i, 3])))
        for k in range(per_sphere):
            d = rng.normal(size=3)
            d /= np.linalg.norm(d)
            side = np.cross(d, rng.normal(size=3))
            side /= np.linalg.norm(side)
            ulps = int(rng.choice([-64, -16, -4, -1, 0, 1, 4, 16, 64]))
            offset = r + ulps * float(np.spacing(np.float32(r)))
            dist = rng.uniform(0.5, 40.0)
            origins.append(c + side * offset - d * dist)  # tangent line at +-ulps
            dirs.append(d)
            if k % 2 == 0:  # an origin on the surface, as a bounce origin is, leaving outward or skimming
                n = rng.normal(size=3)
                n /= np.linalg.norm(n)
                origins.append(c + n * r)
                t = rng.normal(size=3)
                dirs.append(t / np.linalg.norm(t))
            else:  # inside
                origins.append(c + rng.normal(size=3) * r * 0.3)
                t = rng.normal(size=3)
                dirs.append(t / np.linalg.norm(t))
    return np.asarray(origins, dtype=np.float32), normalised(dirs)


@pytest.mark.parametrize("count,seed", [(300, 1), (1500, 2), (5000, 3)])
def test_closest_hit_on_adversarial_rays(tracer, count, seed):
    rng = np.random.default_rng(seed)
    spheres = sphere_field(rng, count)
    # duplicates of some spheres far apart in the index order (different leaves): the lower index must win; nested spheres
    for j in range(20):
        spheres.append(spheres[1 + j * 7])
        x, y, z, r, m = spheres[2 + j * 11]
        spheres.append((x, y, z, r * 0.5, m))
    planes = [(0, 1, 0, 0.5, 2)] if seed % 2 else []
    pod = rt_amd.scene_from_arrays(spheres, planes, MATERIALS)
    origins, dirs = adversarial_rays(spheres, rng)
    # the ground sphere, from above and grazing; degenerate directions
    extra_o = np.array([(0, 2, 0), (5, 0.01, -3), (0, 1, 5), (0, 1, 5), (0, 1, 5), (1, 1, 1)], dtype=np.float32)
    extra_d = np.array([(0, -1, 0), (1, 0, 0), (np.nan, 0, 0), (np.inf, 0, 0), (0, 0, 0), (0, 0, -1)], dtype=np.float32)
    extra_d[[0, 1, 5]] = normalised(extra_d[[0, 1, 5]])
    origins, dirs = np.concatenate([origins, extra_o]), np.concatenate([dirs, extra_d])
    linear = same_hits(tracer, pod, origins, dirs, f"{count} spheres")
    assert (linear[1] == 1).mean() > 0.3  # the rays do hit spheres


def test_duplicate_spheres_in_different_leaves_lower_index_wins(tracer):
    spheres = [(float(i % 40), 0.0, -float(i // 40), 0.2, 0) for i in range(400)]
    spheres += [(5.0, 0.0, -3.0, 0.2, 0)] * 3  # indices 400..402 duplicate sphere 125
    pod = rt_amd.scene_from_arrays(spheres, [], MATERIALS[:1])
    origins = np.array([(5.0, 5.0, -3.0), (5.0, 0.0, 5.0)], dtype=np.float32)
    dirs = normalised([(0, -1, 0), (0, 0, -1)])
    dist, kind, index, _ = same_hits(tracer, pod, origins, dirs, "duplicates")
    assert index[0] == 125 and kind[0] == 1


def test_non_finite_spheres_and_rays(tracer):
    spheres = [(np.nan, 0, -5, 1, 0), (0, 0, -5, np.inf, 0)] + [(float(i), 0.0, -6.0, 0.4, 0) for i in range(-10, 10)]
    pod = rt_amd.scene_from_arrays(spheres, [], MATERIALS[:1])
    rng = np.random.default_rng(5)
    origins = rng.uniform(-3, 3, (500, 3)).astype(np.float32)
    dirs = normalised(rng.normal(size=(500, 3)) + (0, 0, -2))
    same_hits(tracer, pod, origins, dirs, "non-finite spheres")


def field_pod(count, seed, width, height, spp, planes=0):
    rng = np.random.default_rng(seed)
    spheres = sphere_field(rng, count)
    plane_rows = [(0, 1, 0, 0.05 * (k + 1), k % len(MATERIALS)) for k in range(planes)]
    camera = rt_amd.Scene.parse("").set_camera((0.0, 4.0, 3.0), (0.0, -0.35, -1.0))
    ivp = camera.describe(width, height).inverse_view_projection[:]
    return rt_amd.scene_from_arrays(spheres, plane_rows, MATERIALS, samples_per_pixel=spp, max_bounces=7, inverse_view_projection=ivp)


@pytest.mark.parametrize("count,planes,seed", [(1, 0, 1), (9, 1, 2), (64, 2, 3), (700, 0, 4), (2000, 3, 5), (5000, 1, 6)])
@pytest.mark.parametrize("flags", [0, SM], ids=["mg", "sm"])
def test_frames_equal_the_linear_frames(tracer, count, planes, seed, flags):
    width, height, spp = 48, 27, 9
    pod = field_pod(count, seed, width, height, spp, planes)
    want_rgba, want_rgb, want_stats = tracer.render(pod, width, height, seed=seed, flags=flags, want_rgb=True)
    got_rgba, got_rgb, stats = tracer.render(pod, width, height, seed=seed, flags=flags | BVH, want_rgb=True)
    assert stats["kernel"] == "bvh"
    assert np.array_equal(got_rgb.view(np.uint32), want_rgb.view(np.uint32)), f"{count} spheres: float mean differs in {(got_rgb != want_rgb).any(axis=-1).sum()} pixels"
    assert np.array_equal(got_rgba, want_rgba)
    assert stats["segments"] == want_stats["segments"] and stats["sphere_tests"] == want_stats["sphere_tests"]
    if count <= 700:  # and the oracle's
        o_rgba, o_rgb, o_stats = oracle.render(pod, width, height, seed=seed, sm_materials=bool(flags & SM))
        assert np.array_equal(got_rgba, o_rgba) and np.array_equal(got_rgb.view(np.uint32), o_rgb.view(np.uint32))
        assert stats["segments"] == o_stats["segments"]


def test_config5_stripe_digest(tracer):
    """Stripe 90 of BASELINE config 5 (100 000 spheres, 1920x1080, 64 spp) with the flag: the committed oracle digest."""
    import torch

    width, height, spp, seed, stripe = 1920, 1080, 64, 1, 90
    pod = rt_amd.Scene.named("synthetic-100k").set_sampling(spp).describe(width, height)
    tracer.upload(pod)
    frame = torch.empty((8, width), dtype=torch.int32, device="cuda:0")
    tracer.render_device(width, height, frame.data_ptr(), seed=seed, flags=BVH, partition=(stripe, 135, 8), stream=torch.cuda.current_stream().cuda_stream)
    stats = tracer.stats()
    assert stats["kernel"] == "bvh"
    entry = json.loads((GOLDEN / "frame_digests.json").read_text())["config5_stripe90"]
    assert (entry["width"], entry["height"], entry["spp"], entry["seed"], entry["partition"]) == (width, height, spp, seed, [stripe, 135, 8])
    rgba = frame.cpu().numpy().view(np.uint32)
    assert hashlib.sha256(np.ascontiguousarray(rgba).tobytes()).hexdigest() == entry["sha256"]
    if "segments" in entry:
        assert stats["segments"] == entry["segments"]


def test_a_moved_sphere_rebuilds_the_tree(tracer):
    width, height, spp = 40, 24, 4
    rng = np.random.default_rng(11)
    spheres = sphere_field(rng, 1200)
    camera = rt_amd.Scene.parse("").set_camera((0.0, 4.0, 3.0), (0.0, -0.35, -1.0))
    ivp = camera.describe(width, height).inverse_view_projection[:]
    first = rt_amd.scene_from_arrays(spheres, [], MATERIALS, samples_per_pixel=spp, max_bounces=5, inverse_view_projection=ivp)
    tracer.render(first, width, height, seed=3, flags=BVH)
    moved = list(spheres)
    moved[1] = (0.0, 1.5, -6.0, 1.2, 1)  # same count, one sphere moved (and grown) into view
    second = rt_amd.scene_from_arrays(moved, [], MATERIALS, samples_per_pixel=spp, max_bounces=5, inverse_view_projection=ivp)
    got, _, stats = tracer.render(second, width, height, seed=3, flags=BVH)
    assert stats["kernel"] == "bvh"
    want, _, _ = tracer.render(second, width, height, seed=3)
    stale, _, _ = tracer.render(first, width, height, seed=3)
    assert not np.array_equal(want, stale)  # the move is visible
    assert np.array_equal(got, want)


def test_multi_member_context(tracer):
    width, height, spp = 64, 40, 5
    pod = field_pod(1500, 21, width, height, spp)
    want, _, _ = tracer.render(pod, width, height, seed=4)
    with rt_amd.HipRayTracer(devices=[0, 0], peer_copy=True) as multi:
        got, _, stats = multi.render(pod, width, height, seed=4, flags=BVH)
        again, _, _ = multi.render(pod, width, height, seed=4, flags=BVH)
    assert np.array_equal(got, want) and np.array_equal(again, want)


def test_refusals_and_the_preview(tracer):
    pod = field_pod(300, 8, 32, 18, 2)
    for force in (capi.RT_HIP_FLAG_FORCE_TILED, capi.RT_HIP_FLAG_FORCE_RESIDENT, capi.RT_HIP_FLAG_FORCE_STREAMED, capi.RT_HIP_FLAG_FAST):
        with pytest.raises(capi.RtHipError) as refused:
            tracer.render(pod, 32, 18, seed=1, flags=BVH | force)
        assert refused.value.status == 5  # RT_HIP_UNSUPPORTED
    preview, _, stats = tracer.render(pod, 32, 18, flags=capi.RT_HIP_FLAG_PREVIEW | BVH)
    assert stats["kernel"] == "preview"
    want, _, _ = tracer.render(pod, 32, 18, flags=capi.RT_HIP_FLAG_PREVIEW)
    assert np.array_equal(preview, want)


def test_plugin_accel_bvh(tmp_path):
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
    for accel in (None, "bvh"):
        out = tmp_path / f"frame_{accel}.ppm"
        env = dict(os.environ, RT_HIP_SEED="5")
        env.pop("RT_HIP_ACCEL", None)
        if accel:
            env["RT_HIP_ACCEL"] = accel
        done = subprocess.run([str(binary), "--renderer", "hip", "--scene", str(scene), "--size", "96x54", "--spp", "4", "--frames", "1", "--out", str(out)], env=env, capture_output=True, text=True, timeout=300)
        assert done.returncode == 0 and "error" not in done.stderr, done.stderr
        outs.append(out.read_bytes())
    assert outs[0] == outs[1]
    assert len(set(outs[0][-3000:])) > 4  # the field is in the picture
