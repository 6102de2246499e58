"""Progressive frames on the GPU (rt_hip_render_progressive, rt_hip_render_pass_device): after EVERY pass the frame is the one-shot
frame of the same scene at samples_per_pixel = samples_done, bit for bit — packed pixels and float mean — with the CPU oracle as the
yardstick and a tolerance of 0.  Frames are 37 x 23: not a multiple of any tile shape, so every pass has tiles that hang over two edges.

One scene per PASS build of the kernels (pinhole LDS scan, general-camera LDS scan, scalar-load scan, the hierarchy, each also under the
sm table where a scene has dielectrics), pass sizes chosen so that both fold paths run (asserted through the CPU plan dump), the frame
beyond the one-shot limit of 4096 samples, restarts, the finished accumulation, the device level on a partition, the refusals, the plug-in."""
import functools
import os
import subprocess

import numpy as np
import pytest

import rt_amd
from oracle import binding as oracle
from rt_amd import capi
from tests import pass_plan
from tests.bvh_cases import MATERIALS, sphere_field
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

BVH = capi.RT_HIP_FLAG_BVH
SM = capi.RT_HIP_FLAG_SM_MATERIALS
W, H = 37, 23
TILTED = ((0.2, 1.2, 3.0), (0.0, -0.15, -1.0))


def field(count, planes, spp, seed, width=W, height=H):
    rng = np.random.default_rng(seed)
    ivp = rt_amd.Scene.parse("").set_camera((0.0, 4.0, 3.0), (0.0, -0.35, -1.0)).describe(width, height).inverse_view_projection[:]
    return rt_amd.scene_from_arrays(sphere_field(rng, count), [(0, 1, 0, 0.05, 2)] * planes, MATERIALS, samples_per_pixel=spp, max_bounces=6, inverse_view_projection=ivp)


def named(name, tilted=False):
    def make(spp, width=W, height=H):
        scene = rt_amd.Scene.named(name).set_sampling(spp)
        if tilted:
            scene.set_camera(*TILTED)
        return scene.describe(width, height)

    return make


# name -> (spp -> the scene at that many samples per pixel, flags, the kernel a pass must report, (scan, planes, general_camera) of its build)
SCENES = {
    "basic": (named("basic"), 0, "resident", (0, 0, 0)),
    "basic_tilted": (named("basic", tilted=True), 0, "resident", (0, 0, 1)),
    "field50": (lambda spp: field(50, 1, spp, 21), 0, "resident", (0, 1, 0)),
    "field300_bvh": (lambda spp: field(300, 0, spp, 22), BVH, "bvh", (-4, 0, 0)),
    "field1500": (lambda spp: field(1500, 0, spp, 23), 0, "bvh", (-4, 0, 0)),
    "dielectric_sm": (named("dielectric"), SM, "resident", (0, 0, 0)),
}
SEED = 5


@functools.lru_cache(maxsize=None)
def reference(name, spp):
    """The oracle's frame of the scene at `spp` samples per pixel: computed once, shared, read-only."""
    make, flags, _, _ = SCENES[name]
    rgba, rgb, stats = oracle.render(make(spp), W, H, seed=SEED, sm_materials=bool(flags & SM))
    rgba.setflags(write=False), rgb.setflags(write=False)
    return rgba, rgb, stats["segments"]


def assert_is_the_one_shot_frame(name, done, rgba, rgb):
    want_rgba, want_rgb, _ = reference(name, done)
    assert np.array_equal(rgb.view(np.uint32), want_rgb.view(np.uint32)), f"{name}: float mean after {done} samples differs from the oracle at spp = {done} in {(rgb != want_rgb).any(axis=-1).sum()} pixels"
    assert np.array_equal(rgba, want_rgba), f"{name}: packed pixels after {done} samples differ from the oracle at spp = {done} in {(rgba != want_rgba).sum()} pixels"


def abandon_the_frame_in_flight(tracer):
    """The session's one context keeps its accumulation from test to test, and a call on a finished one launches nothing: one pass of
    a frame that no test renders (8 x 8, a seed of its own) leaves a key that differs from every test's, so the next call restarts."""
    tracer.render_progressive(SCENES["basic"][0](16, 8, 8), 8, 8, seed=SEED + 1000, pass_samples=16)


def run_passes(tracer, name, spp, sizes):
    """Pass after pass (sizes: the pass_samples of the calls, the last one repeated) until complete; every frame against the oracle.
    Starts a new accumulation whatever an earlier test left.  Returns the last frame and the passes' stats."""
    make, flags, kernel, _ = SCENES[name]
    pod = make(spp)
    abandon_the_frame_in_flight(tracer)
    done, calls, all_stats = 0, 0, []
    while done < spp:
        size = sizes[min(calls, len(sizes) - 1)]
        rgba, rgb, stats, progress = tracer.render_progressive(pod, W, H, seed=SEED, flags=flags, pass_samples=size, want_rgb=True)
        left = spp - done
        this = left if size == 0 else min(-(-size // 16) * 16, left)
        assert progress == {"samples_done": done + this, "samples_total": spp, "passes": calls + 1, "restarted": 1 if calls == 0 else 0}, (name, size, progress)
        assert stats["kernel"] == kernel and stats["primary_samples"] == W * H * this, (name, stats)
        done, calls = done + this, calls + 1
        assert_is_the_one_shot_frame(name, done, rgba, rgb)
        all_stats.append(stats)
    return rgba, rgb, all_stats


def expected_tiles(name, spp, size):
    """pixels_log2 of a pass of `size` samples, from the CPU plan dump (the launch the drop-in call makes: a host frame)."""
    assert pass_plan.executable() is not None, "the plan dump program needs g++: without it nothing says which fold path a pass takes"
    make, flags, _, build = SCENES[name]
    pod = make(spp)
    camera = 0 if build[2] == 0 and build[0] == 0 and build[1] == 0 else 2
    (plan,) = pass_plan.plans([(pod.n_spheres, pod.n_planes, 1, W, H, spp, camera, flags & (BVH | SM), 1, 0, 0, size)])
    assert (plan["scan"], plan["planes"]) == build[:2] and plan["pass"] == 1
    return plan["pixels_log2"]


@pytest.mark.parametrize("size,pixels_log2", [(16, 6), (32, 5), (48, 4)])
def test_every_pass_of_100_samples_is_the_one_shot_frame(tracer, size, pixels_log2):
    """Six chunks and a 4-sample tail.  Passes of 16 and 32 samples fold per pixel (tiles of 64 and 32), passes of 48 one channel per lane (16)."""
    assert expected_tiles("basic", 100, size) == pixels_log2  # a change of tile policy must not silently drop a fold path
    assert (3 << pixels_log2 <= 64) == (size == 48)
    rgba, rgb, stats = run_passes(tracer, "basic", 100, [size])
    assert len(stats) == -(-100 // size)
    assert sum(s["segments"] for s in stats) == reference("basic", 100)[2]


def test_mixed_pass_sizes(tracer):
    """16, then 48, then all that is left: 16 + 48 + 36."""
    _, _, stats = run_passes(tracer, "basic", 100, [16, 48, 0])
    assert [s["primary_samples"] // (W * H) for s in stats] == [16, 48, 36]


@pytest.mark.parametrize("name,spp,size", [("basic_tilted", 40, 16), ("field50", 40, 16), ("field300_bvh", 40, 16), ("field1500", 40, 16), ("dielectric_sm", 40, 16), ("dielectric_sm", 100, 48)])
def test_one_scene_per_pass_build(tracer, name, spp, size):
    """... and the final frame is rt_hip_render's, the passes' segments sum to its segments."""
    make, flags, kernel, build = SCENES[name]
    if name != "basic_tilted":
        expected_tiles(name, spp, size)  # (asserts the build's scan)
    rgba, rgb, stats = run_passes(tracer, name, spp, [size])
    one_rgba, one_rgb, one_stats = tracer.render(make(spp), W, H, seed=SEED, flags=flags, want_rgb=True)
    assert np.array_equal(rgba, one_rgba) and np.array_equal(rgb.view(np.uint32), one_rgb.view(np.uint32))
    assert sum(s["segments"] for s in stats) == one_stats["segments"] == reference(name, spp)[2]
    if name == "basic_tilted":  # (what makes it the general-camera build: the frame is not a pinhole's)
        assert oracle.primary_ray(make(spp), W, H, 0, 0, want_form=True)[2] != "pinhole"


def test_beyond_the_one_shot_limit(tracer):
    """5000 samples per pixel: rt_hip_render refuses (a pixel's chunk sums must fit one wave's LDS slots), passes of 512 complete."""
    width = height = 8
    pod = rt_amd.Scene.named("basic").set_sampling(5000).describe(width, height)
    with pytest.raises(rt_amd.RtHipError) as refused:
        tracer.render(pod, width, height, seed=SEED)
    assert refused.value.status == 5
    progress = {"samples_done": 0}
    while progress["samples_done"] < 5000:
        rgba, rgb, stats, progress = tracer.render_progressive(pod, width, height, seed=SEED, pass_samples=512, want_rgb=True)
    assert progress["passes"] == 10 and progress["samples_done"] == 5000
    want_rgba, want_rgb, _ = oracle.render(pod, width, height, seed=SEED)
    assert np.array_equal(rgb.view(np.uint32), want_rgb.view(np.uint32)) and np.array_equal(rgba, want_rgba)
    # one pass that does not fit is refused, and says so
    with pytest.raises(rt_amd.RtHipError) as too_large:
        tracer.render_progressive(rt_amd.Scene.named("basic").set_sampling(9000).describe(width, height), width, height, seed=SEED, pass_samples=0)
    assert too_large.value.status == 5 and "pass" in str(too_large.value)


def test_anything_the_frame_depends_on_restarts(tracer):
    """A changed seed, one changed sphere radius, a changed matrix and a changed size: restarted = 1, samples_done = one pass, and the
    frame is the new frame's first pass — nothing of the 32 samples of the other frame that were in flight."""
    spheres = sphere_field(np.random.default_rng(31), 20)
    grown = list(spheres)
    grown[3] = tuple(grown[3][:3]) + (grown[3][3] * 1.5,) + tuple(grown[3][4:])
    camera = rt_amd.Scene.parse("").set_camera((0.0, 4.0, 3.0), (0.0, -0.35, -1.0)).describe(W, H).inverse_view_projection[:]
    moved = rt_amd.Scene.parse("").set_camera((0.1, 4.0, 3.0), (0.0, -0.3, -1.0)).describe(W, H).inverse_view_projection[:]
    base = dict(rows=spheres, matrix=camera, width=W, seed=SEED)
    abandon_the_frame_in_flight(tracer)

    def call(spp=64, **frame):
        pod = rt_amd.scene_from_arrays(frame["rows"], [(0, 1, 0, 0.05, 2)], MATERIALS, samples_per_pixel=spp, max_bounces=5, inverse_view_projection=frame["matrix"])
        return pod, tracer.render_progressive(pod, frame["width"], H, seed=frame["seed"], pass_samples=16, want_rgb=True)

    for change in ({"seed": SEED + 1}, {"rows": grown}, {"matrix": moved}, {"width": W + 1}):
        for expected in ({"samples_done": 16, "passes": 1, "restarted": 1}, {"samples_done": 32, "passes": 2, "restarted": 0}):  # the frame in flight
            _, (_, _, _, progress) = call(**base)
            assert {k: progress[k] for k in expected} == expected, (change.keys(), progress)
        changed = dict(base, **change)
        _, (rgba, rgb, _, progress) = call(**changed)
        assert progress == {"samples_done": 16, "samples_total": 64, "passes": 1, "restarted": 1}, (change.keys(), progress)
        pod16 = rt_amd.scene_from_arrays(changed["rows"], [(0, 1, 0, 0.05, 2)], MATERIALS, samples_per_pixel=16, max_bounces=5, inverse_view_projection=changed["matrix"])
        want_rgba, want_rgb, _ = oracle.render(pod16, changed["width"], H, seed=changed["seed"])
        assert np.array_equal(rgba, want_rgba) and np.array_equal(rgb.view(np.uint32), want_rgb.view(np.uint32)), change.keys()


def test_a_call_after_completion_launches_nothing_and_delivers_the_frame(tracer):
    _, flags, _, _ = SCENES["basic"]
    pod = SCENES["basic"][0](40)
    run_passes(tracer, "basic", 40, [16])
    garbage = np.full((H, W), 0xDEADBEEF, dtype=np.uint32)
    rgba, rgb, stats, progress = tracer.render_progressive(pod, W, H, seed=SEED, flags=flags, pass_samples=16, want_rgb=True, out=garbage)
    assert progress == {"samples_done": 40, "samples_total": 40, "passes": 3, "restarted": 0}
    assert stats["primary_samples"] == 0 and stats["segments"] == 0 and stats["kernel"] == "none"
    assert rgba is garbage
    assert_is_the_one_shot_frame("basic", 40, rgba, rgb)


def test_device_level_passes_on_a_partition(tracer):
    import torch

    width, height, spp, part = 37, 40, 40, (1, 3, 8)
    pod = rt_amd.Scene.named("basic").set_sampling(spp).describe(width, height)
    rows, padded = rt_amd.local_rows(height, *part), rt_amd.padded_local_rows(height, part[1], part[2])
    tracer.upload(pod)
    stream = torch.cuda.current_stream().cuda_stream
    accum = torch.full((padded, width, 3), float("nan"), dtype=torch.float32, device="cuda:0")  # (pass 0 must not read it)
    frame = torch.zeros((padded, width), dtype=torch.int32, device="cuda:0")
    mean = torch.zeros((padded, width, 3), dtype=torch.float32, device="cuda:0")
    mine = [y for y in range(height) if (y // part[2]) % part[1] == part[0]]
    assert len(mine) == rows
    for first, n in ((0, 16), (16, 24)):
        # (the second pass with RT_HIP_FLAG_STATS: both entry points take it, and it changes nothing at this level)
        tracer.render_pass_device(width, height, first, n, accum.data_ptr(), frame.data_ptr(), seed=SEED, flags=capi.RT_HIP_FLAG_STATS if first else 0, partition=part, d_rgb_f32=mean.data_ptr(), stream=stream)
        stats = tracer.stats()
        assert stats["kernel"] == "resident" and stats["primary_samples"] == rows * width * n
        whole = rt_amd.Scene.named("basic").set_sampling(first + n).describe(width, height)
        want_rgba, want_rgb, _ = oracle.render(whole, width, height, seed=SEED)
        assert np.array_equal(frame.cpu().numpy().view(np.uint32)[:rows], want_rgba[mine])
        assert np.array_equal(mean.cpu().numpy().view(np.uint32)[:rows], want_rgb[mine].view(np.uint32))
    # samples that are no whole chunks, or do not lie within the scene's, are refused
    for first, n in ((8, 16), (0, 8), (32, 16), (48, 16), (0, 0)):
        with pytest.raises(rt_amd.RtHipError) as refused:
            tracer.render_pass_device(width, height, first, n, accum.data_ptr(), frame.data_ptr(), seed=SEED, partition=part, stream=stream)
        assert refused.value.status == 1, (first, n)


@pytest.mark.parametrize("flag", ["FAST", "PREVIEW", "FORCE_TILED", "FORCE_RESIDENT", "FORCE_STREAMED", "FORCE_HALF_CHUNKS", "FORCE_WHOLE_CHUNKS", "PERSISTENT_FRAME"])
def test_refused_flags_are_named(tracer, flag):
    import torch

    pod = SCENES["basic"][0](32)
    with pytest.raises(rt_amd.RtHipError) as refused:
        tracer.render_progressive(pod, W, H, seed=SEED, flags=getattr(capi, "RT_HIP_FLAG_" + flag))
    assert refused.value.status == 5 and "RT_HIP_FLAG_" + flag in str(refused.value)
    tracer.upload(pod)
    accum = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda:0")
    frame = torch.zeros((H, W), dtype=torch.int32, device="cuda:0")
    with pytest.raises(rt_amd.RtHipError) as refused:
        tracer.render_pass_device(W, H, 0, 16, accum.data_ptr(), frame.data_ptr(), flags=getattr(capi, "RT_HIP_FLAG_" + flag))
    assert refused.value.status == 5 and "RT_HIP_FLAG_" + flag in str(refused.value)


def test_a_multi_context_is_refused():
    with rt_amd.HipRayTracer(devices=[0], peer_copy=True) as multi:
        with pytest.raises(rt_amd.RtHipError) as refused:
            multi.render_progressive(SCENES["basic"][0](32), W, H, seed=SEED)
        assert refused.value.status == 5 and "rt_hip_create" in str(refused.value)


def test_the_plug_in_in_passes_writes_the_same_file(tmp_path):
    """rt_headless --progressive 16: ceil(spp / 16) calls of render(), the last frame is the one-shot frame of the same seed."""
    binary = ROOT / "rt_amd" / "bin" / "rt_headless"
    common = ["--renderer", "hip", "--scene", "basic.toml", "--size", "37x23", "--spp", "40"]
    env = dict(os.environ, RT_HIP_SEED="7")
    env.pop("RT_HIP_PROGRESSIVE", None)
    files = []
    for extra in ([], ["--progressive", "16"]):
        out = tmp_path / f"frame{len(files)}.ppm"
        done = subprocess.run([str(binary), *common, *extra, "--out", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=300, env=env)
        assert done.returncode == 0 and "error" not in done.stderr, done.stderr
        files.append(out.read_bytes())
    assert len(files[0]) > 37 * 23 * 3 and files[0] == files[1]
    assert rt_amd.live_frame_locks() == 0
