"""Adaptive sampling on the GPU (rt_hip_render_adaptive, rt_hip_adaptive_pass_device, rt_hip_adaptive_update_device).

THE PROMISE: after EVERY pass, pixel (x, y) of the float mean and of the packed frame is the oracle's pixel at samples_per_pixel =
n(x, y), the sample map the call returns — compared as uint32, tolerance 0.  THE DECISIONS: moments and state words after every pass
equal the serial CPU restatement (tests/native/adaptive_reference.cpp) replayed from the previous pass's words and this pass's own
fold, bit for bit; a stopped pixel's words are never touched; the first pass reads nothing.  Frames are 37 x 23: not a multiple of any
tile shape, so tiles — the render kernels' and the update kernel's 16 x 16 — hang over two edges."""
import os
import subprocess

import numpy as np
import pytest

import rt_amd
from rt_amd import capi
from tests import adaptive_plan
from tests import adaptive_reference as ref
from tests.conftest import ROOT
from tests.test_gpu_progressive import BVH, H, SCENES, SEED, SM, W, reference

pytestmark = pytest.mark.gpu

STOPPED, COUNT = ref.STOPPED, ref.COUNT
P = W * H


def abandon_the_accumulation_in_flight(tracer):
    """The session's one context keeps its adaptive accumulation from test to test, and a call on a complete one launches nothing: one
    pass of a frame that no test renders (8 x 8, a seed of its own) leaves a key that differs from every test's."""
    tracer.render_adaptive(SCENES["basic"][0](16, 8, 8), 8, 8, seed=SEED + 1000, pass_samples=16)


def assert_every_pixel_is_the_oracles_at_its_own_count(name, counts, rgba, rgb):
    for s in np.unique(counts):
        want_rgba, want_rgb, _ = reference(name, int(s))
        at = counts == s
        assert np.array_equal(rgb[at].view(np.uint32), want_rgb[at].view(np.uint32)), f"{name}: float mean differs from the oracle at spp = {s} in {(rgb[at] != want_rgb[at]).any(axis=-1).sum()} of {at.sum()} pixels holding {s} samples"
        assert np.array_equal(rgba[at], want_rgba[at]), f"{name}: packed pixels differ from the oracle at spp = {s} in {(rgba[at] != want_rgba[at]).sum()} of {at.sum()} pixels holding {s} samples"


def run_adaptive(tracer, name, cap, size=16, p=None):
    """Pass after pass until complete, every frame against the oracle; -> (rgba, rgb, counts, the passes' stats, the last info)."""
    make, flags, kernel, _ = SCENES[name]
    pod = make(cap)
    abandon_the_accumulation_in_flight(tracer)
    all_stats, previous_counts, calls, traced = [], None, 0, 0
    while True:
        rgba, rgb, counts, stats, info = tracer.render_adaptive(pod, W, H, seed=SEED, flags=flags, pass_samples=size, params=p, want_rgb=True)
        calls += 1
        this = min(size, cap - size * (calls - 1))
        assert info["restarted"] == (1 if calls == 1 else 0) and info["passes"] == calls and info["samples_total"] == cap and info["pixels"] == P, info
        assert info["samples_done"] == counts.max() == size * (calls - 1) + this, (info, counts.max())
        assert stats["kernel"] == kernel, stats
        traced += int(stats["primary_samples"])
        assert info["samples_traced"] == counts.sum() == traced, (info, counts.sum(), traced)
        if previous_counts is not None:  # stopping is monotone: a pixel either got this pass's samples or was left alone
            grew = counts != previous_counts
            assert (counts[grew] == previous_counts[grew] + this).all() and stats["primary_samples"] == int(grew.sum()) * this
            assert info["active_pixels"] <= int(grew.sum())
        assert_every_pixel_is_the_oracles_at_its_own_count(name, counts, rgba, rgb)
        all_stats.append(stats)
        previous_counts = counts
        assert info["complete"] == (1 if info["active_pixels"] == 0 or info["samples_done"] == cap else 0), info
        if info["complete"]:
            return rgba, rgb, counts, all_stats, info
        assert calls < 1000


def tile_of(name, cap, size):
    """pixels_log2 of an adaptive pass of `size` samples, from the CPU plan dump."""
    assert adaptive_plan.executable() is not None, "the plan dump program needs g++: without it nothing says which fold path a pass takes"
    make, flags, _, build = SCENES[name]
    pod = make(cap)
    camera = 0 if build == (0, 0, 0) else 2
    (plan,) = adaptive_plan.plans([(pod.n_spheres, pod.n_planes, 1, W, H, cap, camera, flags & (BVH | SM), 0, size)])
    assert (plan["scan"], plan["planes"]) == build[:2] and plan["adaptive"] == 1
    return plan["pixels_log2"]


# ---- 1. the promise, and 5. work really drops -----------------------------------------------------------------------------------------
def test_the_promise_on_basic_at_the_defaults_and_the_work_drops(tracer):
    """Cap 128, passes of 16, default parameters.  The map must be mixed, or the test shows nothing (a CPU simulation gives 592 pixels
    at 32, 174 at 128 and 7 distinct values)."""
    assert tile_of("basic", 128, 16) == 6  # 64 pixels: the per-pixel fold
    rgba, rgb, counts, stats, info = run_adaptive(tracer, "basic", 128)
    print("sample map:", dict(zip(*np.unique(counts, return_counts=True))))
    assert (counts == 32).sum() >= 100 and (counts == 128).sum() >= 100 and len(np.unique(counts)) >= 4, dict(zip(*np.unique(counts, return_counts=True)))
    assert info["samples_traced"] == counts.sum()
    # the progressive run of the same frame, pass for pass
    pod = SCENES["basic"][0](128)
    tracer.render_progressive(SCENES["basic"][0](16, 8, 8), 8, 8, seed=SEED + 1000, pass_samples=16)
    progressive_segments, done = 0, 0
    while done < 128:
        _, _, s, progress = tracer.render_progressive(pod, W, H, seed=SEED, pass_samples=16)
        progressive_segments, done = progressive_segments + s["segments"], progress["samples_done"]
    adaptive_segments = sum(s["segments"] for s in stats)
    print("segments: adaptive", adaptive_segments, "progressive", progressive_segments)
    assert adaptive_segments < progressive_segments == reference("basic", 128)[2]


def test_the_promise_in_passes_of_48_through_the_channel_per_lane_fold(tracer):
    assert tile_of("basic", 144, 48) == 4 and 3 << 4 <= 64  # 16 pixels: one channel per lane
    _, _, counts, stats, info = run_adaptive(tracer, "basic", 144, 48, ref.params(min_samples=96))
    assert info["passes"] == 3 and set(np.unique(counts)) == {96, 144}, dict(zip(*np.unique(counts, return_counts=True)))


@pytest.mark.parametrize("name", ["basic_tilted", "field50", "field300_bvh", "field1500", "dielectric_sm"])
def test_the_promise_on_one_scene_per_adaptive_build(tracer, name):
    if name != "basic_tilted":
        tile_of(name, 64, 16)  # (asserts the build's scan)
    _, _, counts, stats, info = run_adaptive(tracer, name, 64)
    assert info["complete"] == 1 and counts.max() <= 64 and counts.min() >= 32


# ---- 2. the decisions, at the device level ---------------------------------------------------------------------------------------------
def test_every_decision_is_the_restatements_and_stopped_pixels_are_never_touched(tracer):
    import torch

    cap = 96
    pod = SCENES["basic"][0](cap)
    tracer.upload(pod)
    stream = torch.cuda.current_stream().cuda_stream
    block = torch.full((9 * P,), float("nan"), dtype=torch.float32, device="cuda:0")  # (pass 0 must read none of it)
    frame = torch.zeros((H, W), dtype=torch.int32, device="cuda:0")
    mean = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda:0")
    active = torch.full((1,), -1, dtype=torch.int32, device="cuda:0")
    nan_pattern = np.uint32(0x7FC0BEEF)

    def words():
        host = block.cpu().numpy().view(np.uint32)
        return host[: 3 * P].reshape(H, W, 3).copy(), host[3 * P : 4 * P].reshape(H, W).copy(), host[4 * P : 7 * P].reshape(H, W, 3).copy(), host[7 * P :].reshape(H, W, 2).copy()

    accum0 = state0 = moments0 = None
    segments, any_stopped = 0, False
    for k in range(cap // 16):
        block[4 * P : 7 * P] = torch.from_numpy(np.full(3 * P, nan_pattern, dtype=np.uint32).view(np.float32)).to("cuda:0")  # the pass must rewrite what it traces
        tracer.adaptive_pass_device(W, H, 16 * k, 16, block.data_ptr(), frame.data_ptr(), seed=SEED, d_rgb_f32=mean.data_ptr(), d_active_pixels=active.data_ptr(), stream=stream)
        torch.cuda.synchronize()
        accum, state, pass_sum, moments = words()
        segments += tracer.stats()["segments"]
        was_stopped = np.zeros((H, W), dtype=bool) if k == 0 else (state0 & STOPPED) != 0
        # the replay: the previous pass's moments and state words, this pass's own fold
        want_moments, want_state, want_rgba, want_rgb, want_active = ref.step(accum.view(np.float32), pass_sum.view(np.float32), np.zeros((H, W, 2), dtype=np.float32) if k == 0 else moments0.view(np.float32),
                                                                              np.zeros((H, W), dtype=np.uint32) if k == 0 else state0, 16, k == 0, True)
        assert np.array_equal(state, want_state), f"pass {k}: {(state != want_state).sum()} state words differ from the restatement"
        assert np.array_equal(moments, want_moments.view(np.uint32)), f"pass {k}: moments differ from the restatement"
        assert int(active.cpu().numpy()[0]) == want_active == int(((state & STOPPED) == 0).sum())
        assert np.array_equal(frame.cpu().numpy().view(np.uint32), want_rgba) and np.array_equal(mean.cpu().numpy().view(np.uint32), want_rgb.view(np.uint32))
        # an active pixel: its pass sum was rewritten, and with one-chunk passes the running sum went on by exactly that chunk
        assert (pass_sum[~was_stopped] != nan_pattern).all()
        if k:
            with np.errstate(all="ignore"):
                assert np.array_equal(accum[~was_stopped], (accum0.view(np.float32)[~was_stopped] + pass_sum.view(np.float32)[~was_stopped]).view(np.uint32))
            # a stopped pixel: neither read nor written
            assert (pass_sum[was_stopped] == nan_pattern).all() and np.array_equal(accum[was_stopped], accum0[was_stopped])
            assert np.array_equal(moments[was_stopped], moments0[was_stopped]) and np.array_equal(state[was_stopped], state0[was_stopped])
            any_stopped = any_stopped or was_stopped.any()
        else:
            assert np.array_equal(accum, pass_sum)  # pass 0: the running sum IS the pass's fold, and nothing of the NaN block was read
            assert not np.isnan(accum.view(np.float32)).any()
        counts = state & COUNT
        for s in np.unique(counts):  # ... and the promise holds at this level too
            want, want_mean, _ = reference("basic", int(s))
            assert np.array_equal(frame.cpu().numpy().view(np.uint32)[counts == s], want[counts == s])
        accum0, state0, moments0 = accum, state, moments
    assert any_stopped and segments < reference("basic", cap)[2]
    # samples that are no whole chunks, or do not lie within the scene's, are refused; so is a partition's context (below) and bad params
    for first, n in ((8, 16), (0, 8), (96, 16), (0, 0)):
        with pytest.raises(rt_amd.RtHipError) as refused:
            tracer.adaptive_pass_device(W, H, first, n, block.data_ptr(), frame.data_ptr(), seed=SEED, stream=stream)
        assert refused.value.status == 1, (first, n)


# ---- 3. the update kernel alone -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,height", [(37, 23), (16, 16)])
def test_the_update_kernel_alone_is_the_restatement(tracer, width, height):
    import torch

    rng = np.random.default_rng(width)
    pixels = width * height
    flat = rng.random((height, width)) < 0.7
    level = rng.uniform(0.1, 1.0, size=(height, width, 3))
    accum = np.zeros((height, width, 3), dtype=np.float32)
    moments = np.full((height, width, 2), np.nan, dtype=np.float32)
    state = np.full((height, width), 0xFFFFFFFF, dtype=np.uint32)
    stream = torch.cuda.current_stream().cuda_stream
    p = ref.params()
    saw_stopped_input = False
    for k, (n, whole) in enumerate([(16, True), (16, True), (16, True), (16, True), (8, False)]):
        pass_sum = (np.where(flat[..., None], level, rng.uniform(0.0, 2.0, size=(height, width, 3))) * n).astype(np.float32)
        if k == 2:
            pass_sum[rng.random((height, width)) < 0.05] = np.nan  # a NaN never converges
        active = np.ones((height, width), dtype=bool) if k == 0 else (state & STOPPED) == 0
        saw_stopped_input = saw_stopped_input or not active.all()
        accum = np.where(active[..., None], pass_sum if k == 0 else accum + pass_sum, accum).astype(np.float32)
        pass_sum[~active] = np.nan  # stale scratch: must not be read
        d_accum, d_pass_sum = torch.from_numpy(accum).to("cuda:0"), torch.from_numpy(pass_sum).to("cuda:0")
        d_moments, d_state = torch.from_numpy(moments.copy()).to("cuda:0"), torch.from_numpy(state.view(np.int32).copy()).to("cuda:0")
        d_rgba, d_rgb = torch.zeros((height, width), dtype=torch.int32, device="cuda:0"), torch.zeros((height, width, 3), dtype=torch.float32, device="cuda:0")
        d_active = torch.full((1,), -1, dtype=torch.int32, device="cuda:0")
        tracer.adaptive_update_device(width, height, n, k == 0, whole, d_accum.data_ptr(), d_pass_sum.data_ptr(), d_moments.data_ptr(), d_state.data_ptr(), d_rgba.data_ptr(), params=p, d_rgb_out=d_rgb.data_ptr(),
                                      d_active_pixels=d_active.data_ptr(), stream=stream)
        torch.cuda.synchronize()
        want_moments, want_state, want_rgba, want_rgb, want_active = ref.step(accum, pass_sum, moments, state, n, k == 0, whole, p)
        got_moments, got_state = d_moments.cpu().numpy(), d_state.cpu().numpy().view(np.uint32)
        assert np.array_equal(got_state, want_state), (k, (got_state != want_state).sum())
        assert np.array_equal(got_moments.view(np.uint32), want_moments.view(np.uint32)), k
        assert np.array_equal(d_rgba.cpu().numpy().view(np.uint32), want_rgba) and np.array_equal(d_rgb.cpu().numpy().view(np.uint32), want_rgb.view(np.uint32)), k
        assert int(d_active.cpu().numpy()[0]) == want_active
        moments, state = want_moments, want_state
    assert saw_stopped_input and ((state & STOPPED) != 0).any() and ((state & STOPPED) == 0).any()
    assert pixels == state.size


# ---- 4. the two ends -------------------------------------------------------------------------------------------------------------------
def test_min_samples_above_the_cap_is_the_progressive_frame(tracer):
    cap = 64
    rgba, rgb, counts, stats, info = run_adaptive(tracer, "basic", cap, 16, ref.params(min_samples=4096))
    assert (counts == cap).all() and info["passes"] == 4 and info["active_pixels"] == P
    one_rgba, one_rgb, one_stats = tracer.render(SCENES["basic"][0](cap), W, H, seed=SEED, want_rgb=True)
    want_rgba, want_rgb, want_segments = reference("basic", cap)
    assert np.array_equal(rgba, one_rgba) and np.array_equal(rgb.view(np.uint32), one_rgb.view(np.uint32))
    assert np.array_equal(rgba, want_rgba) and np.array_equal(rgb.view(np.uint32), want_rgb.view(np.uint32))
    assert sum(s["segments"] for s in stats) == want_segments == one_stats["segments"]


def test_a_huge_threshold_stops_every_pixel_after_the_second_pass(tracer):
    cap = 128
    pod = SCENES["basic"][0](cap)
    rgba, rgb, counts, stats, info = run_adaptive(tracer, "basic", cap, 16, ref.params(threshold=1e30))
    assert (counts == 32).all() and info["complete"] == 1 and info["passes"] == 2 and info["active_pixels"] == 0 and info["samples_traced"] == 32 * P
    want_rgba, want_rgb, _ = reference("basic", 32)
    assert np.array_equal(rgba, want_rgba) and np.array_equal(rgb.view(np.uint32), want_rgb.view(np.uint32))
    # the next call launches nothing, delivers the same frame into a garbage-filled buffer and reports zero work
    garbage = np.full((H, W), 0xDEADBEEF, dtype=np.uint32)
    again_rgba, again_rgb, again_counts, again_stats, again = tracer.render_adaptive(pod, W, H, seed=SEED, pass_samples=16, params=ref.params(threshold=1e30), want_rgb=True, out=garbage)
    assert again_rgba is garbage and np.array_equal(again_rgba, want_rgba) and np.array_equal(again_rgb.view(np.uint32), want_rgb.view(np.uint32)) and (again_counts == 32).all()
    assert again_stats["primary_samples"] == 0 and again_stats["segments"] == 0 and again_stats["kernel"] == "none" and again_stats["render_ms"] == 0
    assert again == dict(info, restarted=0)


# ---- 6. restarts, refusals and the plug-in ---------------------------------------------------------------------------------------------
def test_anything_the_accumulation_depends_on_restarts(tracer):
    from tests.bvh_cases import MATERIALS, sphere_field

    spheres = sphere_field(np.random.default_rng(31), 20)
    grown = list(spheres)
    grown[3] = tuple(grown[3][:3]) + (grown[3][3] * 1.5,) + tuple(grown[3][4:])
    camera = rt_amd.Scene.parse("").set_camera((0.0, 4.0, 3.0), (0.0, -0.35, -1.0)).describe(W, H).inverse_view_projection[:]
    moved = rt_amd.Scene.parse("").set_camera((0.1, 4.0, 3.0), (0.0, -0.3, -1.0)).describe(W, H).inverse_view_projection[:]
    base = dict(rows=spheres, matrix=camera, width=W, seed=SEED, threshold=0.03, size=16)
    abandon_the_accumulation_in_flight(tracer)

    def call(**frame):
        pod = rt_amd.scene_from_arrays(frame["rows"], [(0, 1, 0, 0.05, 2)], MATERIALS, samples_per_pixel=96, max_bounces=5, inverse_view_projection=frame["matrix"])
        return tracer.render_adaptive(pod, frame["width"], H, seed=frame["seed"], pass_samples=frame["size"], params=ref.params(threshold=frame["threshold"], min_samples=64), want_rgb=True)

    for change in ({"seed": SEED + 1}, {"rows": grown}, {"matrix": moved}, {"width": W + 1}, {"threshold": 0.04}, {"size": 32}):
        for expected in ({"samples_done": 16, "passes": 1, "restarted": 1}, {"samples_done": 32, "passes": 2, "restarted": 0}):  # the accumulation in flight
            info = call(**base)[4]
            assert {k: info[k] for k in expected} == expected, (change.keys(), info)
        changed = dict(base, **change)
        rgba, rgb, counts, _, info = call(**changed)
        first = changed["size"]
        assert {k: info[k] for k in ("samples_done", "passes", "restarted")} == {"samples_done": first, "passes": 1, "restarted": 1}, (change.keys(), info)
        assert (counts == first).all()
        pod = rt_amd.scene_from_arrays(changed["rows"], [(0, 1, 0, 0.05, 2)], MATERIALS, samples_per_pixel=first, max_bounces=5, inverse_view_projection=changed["matrix"])
        from oracle import binding as oracle

        want_rgba, want_rgb, _ = oracle.render(pod, changed["width"], H, seed=changed["seed"])
        assert np.array_equal(rgba, want_rgba) and np.array_equal(rgb.view(np.uint32), want_rgb.view(np.uint32)), change.keys()


@pytest.mark.parametrize("flag", ["FAST", "PREVIEW", "FORCE_TILED", "FORCE_RESIDENT", "FORCE_STREAMED", "FORCE_HALF_CHUNKS", "FORCE_WHOLE_CHUNKS", "PERSISTENT_FRAME", "TRACE_BOXES", "BOX_BVH"])
def test_refused_flags_are_named(tracer, flag):
    import torch

    pod = SCENES["basic"][0](64)
    with pytest.raises(rt_amd.RtHipError) as refused:
        tracer.render_adaptive(pod, W, H, seed=SEED, flags=getattr(capi, "RT_HIP_FLAG_" + flag))
    assert refused.value.status == 5 and "RT_HIP_FLAG_" + flag in str(refused.value)
    tracer.upload(pod)
    block = torch.zeros((9 * P,), dtype=torch.float32, device="cuda:0")
    frame = torch.zeros((H, W), dtype=torch.int32, device="cuda:0")
    with pytest.raises(rt_amd.RtHipError) as refused:
        tracer.adaptive_pass_device(W, H, 0, 16, block.data_ptr(), frame.data_ptr(), flags=getattr(capi, "RT_HIP_FLAG_" + flag))
    assert refused.value.status == 5 and "RT_HIP_FLAG_" + flag in str(refused.value)


def test_a_multi_context_is_refused():
    with rt_amd.HipRayTracer(devices=[0], peer_copy=True) as multi:
        with pytest.raises(rt_amd.RtHipError) as refused:
            multi.render_adaptive(SCENES["basic"][0](64), W, H, seed=SEED)
        assert refused.value.status == 5 and "rt_hip_create" in str(refused.value)


def test_the_plug_in_runs_an_adaptive_accumulation_to_completion(tmp_path):
    """rt_headless --adaptive: render() until complete (the driver asks rt_hip_adaptive_last_info), the last frame written, the samples
    traced printed against pixels x spp, and the process's rt_hip_live_frame_locks() — 0 — reported by the process itself."""
    binary = ROOT / "rt_amd" / "bin" / "rt_headless"
    env = dict(os.environ, RT_HIP_SEED="7")
    for name in ("RT_HIP_PROGRESSIVE", "RT_HIP_ADAPTIVE", "RT_HIP_TEMPORAL"):
        env.pop(name, None)
    out = tmp_path / "frame.ppm"
    done = subprocess.run([str(binary), "--renderer", "hip", "--scene", "basic.toml", "--size", "37x23", "--spp", "128", "--adaptive", "0.03", "--out", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=300, env=env)
    assert done.returncode == 0 and "error" not in done.stderr, done.stderr
    (line,) = [l for l in done.stdout.splitlines() if l.startswith("adaptive: complete")]
    fields = line.replace("=", " ").split()
    traced, budget = int(fields[fields.index("samples_traced") + 1]), int(fields[fields.index("spp") + 1])
    assert budget == P * 128 and 32 * P <= traced < budget, line
    assert len(out.read_bytes()) > P * 3
    assert "adaptive: live frame locks 0" in done.stdout.splitlines()  # (the child's own count, printed when its accumulation is complete)
