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
from rt_amd.renderer import bvh_build
from tests import bvh_cases
from tests.bvh_cases import MATERIALS, adversarial_rays, normalised, sphere_field
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu

BVH = capi.RT_HIP_FLAG_BVH
SM = capi.RT_HIP_FLAG_SM_MATERIALS
ROOT = __import__("pathlib").Path(__file__).resolve().parent.parent

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


@pytest.mark.parametrize("count,planes,seed", [(1, 0, 1), (2, 0, 7), (3, 1, 8), (5, 0, 9), (6, 1, 10), (9, 1, 2), (64, 2, 3), (700, 0, 4), (2000, 3, 5), (5000, 1, 6)])
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


# ---- the regimes of tests/bvh_cases.py: scale, far origins, off-centre scenes, underflow, duplicates, axis rays ------------
@pytest.mark.parametrize("name", list(bvh_cases.REGIMES))
def test_closest_hit_in_every_regime_of_the_cull_bound(tracer, name):
    """The scenes and rays of the CPU audit (tests/test_bvh_cull_audit.py) through the compiled traversal."""
    for label, rows, origins, dirs in bvh_cases.regime_cases(name):
        assert len(origins) <= 1 << 20
        pod = bvh_cases.sphere_scene(rows)
        assert len(bvh_build(pod)["order"]) == len(rows)  # every sphere is in the tree
        same_hits(tracer, pod, origins, dirs, f"{name} / {label}")


GATE_FACTORS = [1 - 2.0**-23, 1 + 2.0**-23, 1 - 2.0**-22, 1 + 2.0**-22, 1 - 3 * 2.0**-23, 1 + 3 * 2.0**-23, 1 - 2.0**-21, 1 + 2.0**-21, 1.0001, 2.0]


def test_directions_at_the_edges_of_the_length_gate(tracer):
    """|d|^2 within 2^-21 of 1 goes through the tree, anything else to the linear scan: the same answer on either side."""
    rng = np.random.default_rng(31)
    spheres = sphere_field(rng, 600)
    pod = rt_amd.scene_from_arrays(spheres, [], MATERIALS)
    origins, dirs = adversarial_rays(spheres, rng)
    origins = np.tile(origins, (len(GATE_FACTORS), 1))
    dirs = np.concatenate([dirs * np.float32(f) for f in GATE_FACTORS])
    dd = bvh_cases.fused_dot(dirs, dirs).astype(np.float64)
    low, high = float(np.float32(1) - np.float32(2.0**-21)), float(np.float32(1) + np.float32(2.0**-21))
    for edge in (low, high):  # rays close to this edge, on both sides of it, and one exactly on it if the batch has one
        close = np.abs(dd - edge) <= 2.0**-22
        assert (dd[close] < edge).sum() >= 100 and (dd[close] > edge).sum() >= 100, f"the batch does not straddle {edge}"
    assert (dd < low).sum() >= 1000 and (dd > high).sum() >= 1000 and ((dd >= low) & (dd <= high)).sum() >= 1000
    linear = same_hits(tracer, pod, origins, dirs, "gate edges")
    assert (linear[1] == 1).mean() > 0.3


# ---- the traversal stack's last word --------------------------------------------------------------------------------------
def axis_rays(axis, sign):
    """Along the cluster axis from beyond the outermost cluster, and small perturbations of origin and direction."""
    along = np.zeros(3)
    along[axis] = sign
    origins, dirs = [-along], [along]
    rng = np.random.default_rng(40 + axis)
    for scale in (1e-7, 1e-5, 1e-4, 1e-3):
        for _ in range(3):
            origins.append(-along + rng.normal(size=3) * scale)
            dirs.append(along)
            origins.append(-along)
            dirs.append(along + rng.normal(size=3) * scale)
            origins.append(-along * rng.uniform(1, 3) + rng.normal(size=3) * scale)
            dirs.append(along + rng.normal(size=3) * scale)
    return np.asarray(origins, dtype=np.float32), normalised(dirs)


def modelled(rows, tree, origins, dirs):
    """Per pad rounding (-4, -1, 0, +1, +4 ulp): per ray (t, index, stack entries in use at most) of the numpy model."""
    answers = bvh_cases.leaf_answers(rows, tree, origins, dirs)
    out = {}
    for ulps in (-4, -1, 0, 1, 4):
        pad = bvh_cases.query_pad(tree, origins, ulps)
        out[ulps] = [bvh_cases.model_traversal(rows, tree, origins[k], dirs[k], k, answers, pad[k]) for k in range(len(origins))]
    return out


@pytest.mark.parametrize("axis,sign", [(0, 1.0), (1, 1.0), (2, 1.0)])
def test_a_ray_that_fills_the_stack(tracer, axis, sign):
    """The depth-24 tree of bvh_cases.cluster_chain and rays that enter both children at every level: the last of the
    bvh_max_depth stack words per lane is written and read back.  That these rays do so is established here, by a numpy model
    of the visiting order (sphere distances from the oracle), with the margin rounded either way."""
    rows = bvh_cases.cluster_chain(axis, sign)
    pod = bvh_cases.sphere_scene(rows)
    tree = bvh_build(pod)
    assert tree["depth"] == bvh_cases.STACK_DEPTH and len(tree["always"]) == 0
    origins, dirs = axis_rays(axis, sign)
    model = modelled(rows, tree, origins, dirs)
    for ulps, rays in model.items():
        depths = [deepest for _, _, deepest in rays]
        print(f"axis {axis} sign {sign:+.0f} pad {ulps:+d} ulp: stack depths {depths}")
        assert depths[0] == bvh_cases.STACK_DEPTH, f"the axis ray uses {depths[0]} stack words with the pad {ulps:+d} ulp"
        assert max(depths) <= bvh_cases.STACK_DEPTH
    dist, kind, index, _ = same_hits(tracer, pod, origins, dirs, f"cluster chain, axis {axis}")
    assert kind[0] == 1  # the axis ray hits (an exact tie in t among the tiny clusters, settled by index)
    for rays in model.values():  # whatever the rounding of the margin, the model's answer is the device's
        for k, (t, i, _) in enumerate(rays):
            assert (t is not None) == (kind[k] == 1)
            if t is not None:
                assert np.float32(t).view(np.uint32) == dist[k].view(np.uint32) and i == index[k], f"ray {k}: model ({t}, {i}), device ({dist[k]}, {index[k]})"


def chain_frame(width, height, spp):
    rows = bvh_cases.cluster_chain(0, 1.0)
    rows[:, 4] = np.arange(len(rows)) % len(MATERIALS)
    camera = rt_amd.Scene.parse("").set_camera((-1.0, 0.0, 0.0), (1.0, 0.0, 0.0))
    ivp = camera.describe(width, height).inverse_view_projection[:]
    planes = [(0, 1, 0, 0.5, 1), (0.6, 0.8, 0, 2.0, 2)]  # so that the tile queue's slots, next to the stacks in LDS, are busy
    return rows, rt_amd.scene_from_arrays(rows, planes, MATERIALS, samples_per_pixel=spp, max_bounces=6, inverse_view_projection=ivp)


@pytest.mark.parametrize("flags", [0, SM], ids=["mg", "sm"])
def test_frames_of_a_tree_as_deep_as_the_stack(tracer, flags):
    """The render kernel's stacks share LDS with the tile queue's slots: a stack that overran would show as wrong sums."""
    width, height, spp = 65, 37, 6
    rows, pod = chain_frame(width, height, spp)
    tree = bvh_build(pod)
    assert tree["depth"] == bvh_cases.STACK_DEPTH
    # the centre pixel's rays run along the axis: its centre ray fills the stack, whichever way the margin is rounded
    o, d = oracle.primary_ray(pod, width, height, width // 2, height // 2)
    for ulps, rays in modelled(rows, tree, o.reshape(1, 3), d.reshape(1, 3)).items():
        assert rays[0][2] == bvh_cases.STACK_DEPTH, f"the centre ray o={o} d={d} uses {rays[0][2]} stack words (pad {ulps:+d} ulp)"
    want_rgba, want_rgb, want_stats = tracer.render(pod, width, height, seed=12, flags=flags, want_rgb=True)
    got_rgba, got_rgb, stats = tracer.render(pod, width, height, seed=12, flags=flags | BVH, want_rgb=True)
    o_rgba, o_rgb, o_stats = oracle.render(pod, width, height, seed=12, sm_materials=bool(flags & SM))
    assert stats["kernel"] == "bvh"
    assert np.array_equal(got_rgb.view(np.uint32), want_rgb.view(np.uint32)) and np.array_equal(got_rgba, want_rgba)
    assert np.array_equal(got_rgb.view(np.uint32), o_rgb.view(np.uint32)) and np.array_equal(got_rgba, o_rgba)
    assert stats["segments"] == want_stats["segments"] == o_stats["segments"]
    assert stats["segments"] > 5 * width * height * spp // 4  # rays do bounce off the planes: the queue is in use


# ---- the render kernel's fall-back to the linear scan ---------------------------------------------------------------------
FALL_BACK = {
    "nan centre": (np.nan, 1.0, -6.0, 0.5, 1),  # every distance to it is a NaN: every lane falls back
    "infinite radius": (0.0, 1.0, -6.0, np.inf, 2),  # every distance to it is infinite: every lane falls back
    # e = c - o has two components of 3e38.  Where d.x - d.z is above 1.134, e . d overflows, the discriminant is a NaN and the
    # lane is reported; elsewhere e . d is finite, e . e is infinite, the discriminant -inf and the sphere simply missed.
    "some lanes": (3e38, 0.0, -3e38, 1.0, 3),
}


def fall_back_pod(kind, count, width, height, spp):
    rng = np.random.default_rng(count)
    spheres = sphere_field(rng, count)
    spheres.insert(count // 2, FALL_BACK[kind])
    camera = rt_amd.Scene.parse("").set_camera((0.0, 4.0, 3.0), (0.0, -0.35, -1.0))
    ivp = camera.describe(width, height).inverse_view_projection[:]
    return rt_amd.scene_from_arrays(spheres, [(0, 1, 0, 0.05, 2)], MATERIALS, samples_per_pixel=spp, max_bounces=7, inverse_view_projection=ivp)


@pytest.mark.parametrize("count", [300, 3000])
@pytest.mark.parametrize("kind", list(FALL_BACK))
@pytest.mark.parametrize("flags", [0, SM], ids=["mg", "sm"])
def test_frames_whose_lanes_fall_back_to_the_linear_scan(tracer, flags, kind, count):
    width, height, spp = 80, 45, 5  # 3600 pixels: many waves' tiles
    pod = fall_back_pod(kind, count, width, height, spp)
    tree = bvh_build(pod)
    assert count // 2 in tree["always"].tolist() and len(tree["order"]) == count - 1
    # which primary rays (pixel centres) meet a non-finite distance at that sphere
    rays = [oracle.primary_ray(pod, width, height, x, y) for y in range(height) for x in range(width)]
    o, d = np.array([r[0] for r in rays]), np.array([r[1] for r in rays])
    with np.errstate(all="ignore"):
        e = np.asarray(FALL_BACK[kind][:3], dtype=np.float32) - o
        reported = ~np.isfinite(bvh_cases.fused_dot(e, d)) | ~np.isfinite(np.float32(FALL_BACK[kind][3]))
    share = reported.reshape(height, width).mean(axis=0)  # per pixel column
    if kind == "some lanes":
        # both kinds of ray, and a boundary that runs down the picture: whatever a wave's tile is, some tiles straddle it
        assert 0.1 < reported.mean() < 0.9, f"{reported.mean():.2f} of the primary rays are reported"
        assert (share == 0).any() and (share == 1).any()
    else:
        assert reported.all()
    want_rgba, want_rgb, want_stats = tracer.render(pod, width, height, seed=5, flags=flags, want_rgb=True)
    got_rgba, got_rgb, stats = tracer.render(pod, width, height, seed=5, flags=flags | BVH, want_rgb=True)
    o_rgba, o_rgb, o_stats = oracle.render(pod, width, height, seed=5, sm_materials=bool(flags & SM))
    assert stats["kernel"] == "bvh"
    for other_rgba, other_rgb, other_stats, name in ((want_rgba, want_rgb, want_stats, "the linear frame"), (o_rgba, o_rgb, o_stats, "the oracle")):
        same = (got_rgb.view(np.uint32) == other_rgb.view(np.uint32)) | (np.isnan(got_rgb) & np.isnan(other_rgb))
        assert same.all(), f"{kind}, {count} spheres: float mean differs from {name} in {(~same).any(axis=-1).sum()} pixels"
        assert np.array_equal(got_rgba, other_rgba), f"{kind}, {count} spheres: packed pixels differ from {name}"
        assert stats["segments"] == other_stats["segments"]


# ---- small trees and long always lists ------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [2, 3, 4, 5, 8])
@pytest.mark.parametrize("flags", [0, SM], ids=["mg", "sm"])
def test_frames_of_small_trees_without_an_always_list(tracer, count, flags):
    """No large sphere: n_always == 0.  Up to four spheres the root link is a leaf; five make the first inner node."""
    width, height, spp = 48, 27, 9
    rng = np.random.default_rng(100 + count)
    # centres 4 apart at the ends: a radius below 1 is not "large" to the builder
    spheres = [(-2 + 4 * k / (count - 1), rng.uniform(0.3, 2), rng.uniform(-6, -3), rng.uniform(0.2, 0.45), int(rng.integers(0, len(MATERIALS)))) for k in range(count)]
    camera = rt_amd.Scene.parse("").set_camera((0.0, 1.5, 3.0), (0.0, -0.1, -1.0))
    ivp = camera.describe(width, height).inverse_view_projection[:]
    pod = rt_amd.scene_from_arrays(spheres, [(0, 1, 0, 0.0, 0)], MATERIALS, samples_per_pixel=spp, max_bounces=7, inverse_view_projection=ivp)
    tree = bvh_build(pod)
    assert len(tree["always"]) == 0 and len(tree["order"]) == count and (len(tree["nodes"]) == 0) == (count <= 4) and (count != 5 or len(tree["nodes"]) == 1)
    want_rgba, want_rgb, want_stats = tracer.render(pod, width, height, seed=count, flags=flags, want_rgb=True)
    got_rgba, got_rgb, stats = tracer.render(pod, width, height, seed=count, flags=flags | BVH, want_rgb=True)
    o_rgba, o_rgb, o_stats = oracle.render(pod, width, height, seed=count, sm_materials=bool(flags & SM))
    assert stats["kernel"] == "bvh"
    assert np.array_equal(got_rgb.view(np.uint32), want_rgb.view(np.uint32)) and np.array_equal(got_rgba, want_rgba)
    assert np.array_equal(got_rgb.view(np.uint32), o_rgb.view(np.uint32)) and np.array_equal(got_rgba, o_rgba)
    assert stats["segments"] == want_stats["segments"] == o_stats["segments"] and stats["sphere_tests"] == want_stats["sphere_tests"]
    assert len(np.unique(got_rgba)) > 50  # the spheres are in the picture


def rays_at(rows, targets, rng, count):
    c, r = bvh_cases.rounded(rows)
    pick = rng.choice(targets, size=count)
    d = bvh_cases.unit(rng.normal(size=(count, 3)))
    aim = c[pick] + rng.uniform(-0.5, 0.5, (count, 3)) * r[pick, None]
    return (aim - d * rng.uniform(30, 60, (count, 1))).astype(np.float32), normalised(d)


def test_an_always_list_at_its_cap_ties_with_the_tree(tracer):
    """Twelve copies of one large sphere, eight in the always list and four in the tree: the lowest index wins the tie."""
    rows, large = bvh_cases.always_cap_identical()
    pod = bvh_cases.sphere_scene(rows)
    tree = bvh_build(pod)
    assert tree["always"].tolist() == large[:8] and set(large[8:]) <= set(tree["order"].tolist())
    rng = np.random.default_rng(51)
    outside_o, outside_d = rays_at(rows, large, rng, 4000)
    near_o, near_d = bvh_cases.near_rays(rows, rng, 4000, 1.0)
    dist, kind, index, _ = same_hits(tracer, pod, np.concatenate([outside_o, near_o]), np.concatenate([outside_d, near_d]), "always list, identical")
    assert (kind[:4000] == 1).all() and (index[:4000] == large[0]).all()


def test_an_always_list_of_the_largest_spheres(tracer):
    rows, large, radii = bvh_cases.always_cap_distinct()
    pod = bvh_cases.sphere_scene(rows)
    tree = bvh_build(pod)
    assert len(tree["always"]) == 8 and set(large) - set(tree["always"].tolist()) <= set(tree["order"].tolist())
    rng = np.random.default_rng(52)
    outside_o, outside_d = rays_at(rows, large, rng, 4000)
    near_o, near_d = bvh_cases.near_rays(rows, rng, 4000, 1.0)
    dist, kind, index, _ = same_hits(tracer, pod, np.concatenate([outside_o, near_o]), np.concatenate([outside_d, near_d]), "always list, distinct")
    outermost = large[int(np.argmax(radii))]  # the spheres are nested: from outside, the largest is met first
    assert (kind[:4000] == 1).all() and (index[:4000] == outermost).all()
