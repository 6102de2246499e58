"""Temporal accumulation on the GPU, tolerance 0 throughout: rt_hip_reproject_device against the serial CPU
restatement over the kernel's own per-pixel text (tests/reproject_reference.py) — every word of the colour and of the record, and the
history count; the drop-in rt_hip_render_temporal against the composition oracle frame -> guide -> reprojection -> (filter) -> pack;
what out_info reports; that the history leaves the context's other state alone; the refusals; and the plug-in through rt_headless.
Frames are at most 96 x 54: 70 x 41 is ragged against the kernel's 32 x 8 tiles (3 x 6 of them, two partial waves in the last row)."""
import functools
import os
import subprocess

import numpy as np
import pytest

import rt_amd
from oracle import binding as oracle
from rt_amd import capi
from tests import denoise_reference as filter_ref
from tests import reproject_reference as ref
from tests import temporal_cases as cases
from tests.conftest import ROOT, unpack
from tests.temporal_cases import bits

pytestmark = pytest.mark.gpu

F32 = np.float32
BOXES = capi.RT_HIP_FLAG_TRACE_BOXES
INVALID_ARGUMENT, UNSUPPORTED = 1, 5


def device_step(tracer, pod, guide, rgb, samples_in, prev=None, p=None, count=True, device_guide_flags=None):
    """rt_hip_reproject_device on copies of the arrays: (rgb, record, pixels with history or None).  device_guide_flags: the guide
    is made on the device with these flags instead (and must be `guide`)."""
    import torch

    height, width = rgb.shape[:2]
    device = f"cuda:{tracer.device}"
    stream = torch.cuda.current_stream().cuda_stream
    tracer.upload(pod)
    to = lambda a: torch.from_numpy(np.array(a, dtype=F32)).to(device)  # noqa: E731  (np.array: a copy, the cached yardsticks are read-only)
    d_guide, d_rgb = to(guide), to(rgb)
    if device_guide_flags is not None:
        d_guide = torch.full((height, width, 8), float("nan"), dtype=torch.float32, device=device)
        tracer.guide_device(width, height, d_guide.data_ptr(), flags=device_guide_flags, stream=stream)
    d_prev_rgb, d_prev_record = (to(prev[1]), to(prev[2])) if prev is not None else (None, None)
    d_out = torch.full((height, width, 3), float("nan"), dtype=torch.float32, device=device)
    d_record = torch.full((height, width, 8), float("nan"), dtype=torch.float32, device=device)
    d_found = torch.full((1,), -7, dtype=torch.int32, device=device)
    tracer.reproject_device(width, height, prev[0] if prev is not None else None, d_guide.data_ptr(), d_rgb.data_ptr(), samples_in, d_prev_rgb.data_ptr() if prev is not None else None, d_prev_record.data_ptr() if prev is not None else None, p,
                            d_out.data_ptr(), d_record.data_ptr(), d_found.data_ptr() if count else None, stream=stream)
    if device_guide_flags is not None:
        assert np.array_equal(bits(d_guide.cpu().numpy()), bits(guide)), "the device's guide is not the composed one"
    assert np.array_equal(bits(d_rgb.cpu().numpy()), bits(rgb))  # (the inputs are not touched)
    if prev is not None:
        assert np.array_equal(bits(d_prev_rgb.cpu().numpy()), bits(prev[1])) and np.array_equal(bits(d_prev_record.cpu().numpy()), bits(prev[2]))
    found = int(d_found.cpu().numpy().view(np.uint32)[0])
    return d_out.cpu().numpy(), d_record.cpu().numpy(), (found if count else None)


def assert_step_is_the_restatement(tracer, pod, guide, rgb, samples_in, prev, p, what, **how):
    got_rgb, got_record, got_found = device_step(tracer, pod, guide, rgb, samples_in, prev, p, **how)
    want_rgb, want_record, want_found = ref.frame(pod, guide, rgb, samples_in, *(prev if prev is not None else (None, None, None)), p)
    differing = (bits(got_rgb) != bits(want_rgb)).any(axis=-1) | (bits(got_record) != bits(want_record)).any(axis=-1)
    assert not differing.any(), f"{what}: {differing.sum()} of {differing.size} pixels differ from the restatement, first at (y, x) = {tuple(np.argwhere(differing)[0])}"
    assert got_found == want_found, what
    return want_rgb, want_record, want_found


# ---- rt_hip_reproject_device against the restatement ------------------------------------------------------------------------------
CHAINED = [("basic:rest", 70, 41), ("basic:dolly", 96, 54), ("basic:yaw", 70, 41), ("basic:about_face", 70, 41), ("basic:dolly", 5, 3), ("basic:rest", 1, 1), ("tilted:dolly", 1, 1), ("tilted:dolly", 70, 41), ("tilted:yaw", 70, 41),
           ("guarded:dolly", 70, 41), ("orthographic:rest", 70, 41), ("orthographic:dolly", 70, 41), ("orthographic:about_face", 70, 41), ("planes_and_sky:dolly", 70, 41), ("planes_and_sky:yaw", 96, 54), ("surround:about_face", 96, 54),
           ("surround_tilted:about_face", 70, 41), ("boxes:dolly", 70, 41), ("boxes:yaw", 70, 41)]


@pytest.mark.parametrize("name,width,height", CHAINED, ids=[f"{n}-{w}x{h}" for n, w, h in CHAINED])
def test_two_chained_frames_are_the_restatements_in_every_word(tracer, name, width, height):
    """Frame 0 has no history (both pointers NULL); frame 1's history is what frame 0 left, under the default parameters."""
    pods, guides, boxes = cases.case(name, width, height)
    how = {"device_guide_flags": BOXES} if boxes else {}
    if boxes:
        assert (ref.ids_of(guides[0]) > pods[0].n_spheres + pods[0].n_planes).any()  # a box in sight: the guide was made under the flag
    first = assert_step_is_the_restatement(tracer, pods[0], guides[0], cases.oracle_mean(pods[0], width, height, 3, boxes), 16, None, None, f"{name} frame 0", **how)
    assert first[2] == 0
    prev = (ref.matrix_of(pods[0]), first[0], first[1])
    second = assert_step_is_the_restatement(tracer, pods[1], guides[1], cases.oracle_mean(pods[1], width, height, 4, boxes), 16, prev, None, f"{name} frame 1", **how)
    hits = int((ref.ids_of(guides[1]) != 0).sum())
    if name.endswith("about_face"):
        assert second[2] == 0 and hits > 0
    elif width * height > 1:
        assert 0 < second[2] <= hits  # (the case says something: history was found)
    if name == "planes_and_sky:dolly":
        assert hits < width * height


def test_the_cases_above_cover_all_three_camera_forms():
    forms = {name: [oracle.primary_ray(pod, width, height, 0, 0, want_form=True)[2] for pod in cases.case(name, width, height)[0]] for name, width, height in CHAINED}
    assert {form for pair in forms.values() for form in pair} == {"pinhole", "eye", "general"}
    assert forms["guarded:dolly"] == ["eye", "eye"] and forms["orthographic:dolly"] == ["general", "general"] and forms["basic:dolly"] == ["pinhole", "pinhole"]
    assert "eye" in forms["tilted:yaw"]  # the plain eye form (guarded:dolly is the guarded one)


def poisoned_history(name, width, height, seed):
    """A history nobody rendered: frame 0's record with its lengths replaced by anything a float can be, some ids and normals
    disturbed, random colours, a NaN pixel and an infinite one."""
    rng = np.random.default_rng(seed)
    matrix, _, record = cases.first_history(name, width, height)
    record = record.copy()
    record[..., 3] = rng.choice(np.array([0.0, -4.0, 0.5, 16.0, 48.0, 1000.0, 3e6, np.inf, np.nan], dtype=F32), size=(height, width))
    ids = ref.ids_of(record).copy()
    disturbed = rng.random((height, width)) < 0.1
    ids[disturbed] = rng.integers(0, 5, size=int(disturbed.sum()))
    record[..., 7] = ids.view(F32)
    record[..., 4:7] += rng.normal(0.0, 0.2, size=(height, width, 3)).astype(F32)
    record[..., 0:3] += (rng.normal(0.0, 0.02, size=(height, width, 3)) * (rng.random((height, width, 1)) < 0.3)).astype(F32)  # (three pixels in ten)
    rgb = rng.uniform(-0.2, 1.5, size=(height, width, 3)).astype(F32)
    rgb[height // 2, width // 3, 0] = np.nan
    rgb[height - 2, width // 2, 2] = np.inf
    return matrix, rgb, record


NON_DEFAULT = [{}, {"max_history_samples": 1, "position_tolerance": 1e-4, "normal_threshold": -1.0}, {"max_history_samples": 1 << 20, "position_tolerance": 0.5, "normal_threshold": 0.2}]


@pytest.mark.parametrize("name,width,height", [("basic:dolly", 70, 41), ("planes_and_sky:dolly", 70, 41), ("orthographic:dolly", 37, 23)])
def test_a_random_history_with_a_nan_and_an_infinite_pixel_under_default_and_other_parameters(tracer, name, width, height):
    pods, guides, _ = cases.case(name, width, height)
    prev = poisoned_history(name, width, height, 31)
    rng = np.random.default_rng(32)
    noise = rng.uniform(0.0, 1.2, size=(height, width, 3)).astype(F32)
    # the tight parameters (a tap must be the very point) meet the history under ITS OWN camera, the others after the move
    for fields, samples_in, k in zip(NON_DEFAULT, (16, 1, 4096), (1, 0, 1)):
        current = noise.copy()
        hit = np.argwhere(ref.ids_of(guides[k]) != 0)
        current[tuple(hit[len(hit) // 2])] = (0.5, np.nan, 0.5)  # a non-finite CURRENT pixel: passes through with length 0
        current[tuple(hit[len(hit) // 3])] = (np.inf, 0.5, 0.5)
        rgb, record, found = assert_step_is_the_restatement(tracer, pods[k], guides[k], current, samples_in, prev, ref.params(**fields), f"{name} {fields}")
        assert found > 0
        assert record[tuple(hit[len(hit) // 2])][3] == 0.0
        finite_in = np.isfinite(current).all(axis=-1)
        assert np.isfinite(rgb[finite_in]).all()  # nothing spread


def test_a_null_count_and_null_params_are_the_defaults_without_a_count(tracer):
    pods, guides, _ = cases.case("basic:dolly", 70, 41)
    prev = cases.first_history("basic:dolly", 70, 41)
    current = cases.oracle_mean(pods[1], 70, 41, 4)
    got_rgb, got_record, got_found = device_step(tracer, pods[1], guides[1], current, 16, prev, None, count=False)
    want_rgb, want_record, _ = ref.frame(pods[1], guides[1], current, 16, *prev, ref.params())
    assert got_found is None and np.array_equal(bits(got_rgb), bits(want_rgb)) and np.array_equal(bits(got_record), bits(want_record))


def test_on_a_multi_context_the_root_member_answers():
    pods, guides, _ = cases.case("basic:dolly", 70, 41)
    with rt_amd.HipRayTracer(devices=[0], peer_copy=True) as multi:
        assert_step_is_the_restatement(multi, pods[1], guides[1], cases.oracle_mean(pods[1], 70, 41, 4), 16, cases.first_history("basic:dolly", 70, 41), None, "multi")


def test_reproject_devices_refusals(tracer):
    import torch

    width, height = 70, 41
    pods, _, _ = cases.case("basic:dolly", width, height)
    tracer.upload(pods[1])
    rgb = [torch.zeros((height, width, 3), dtype=torch.float32, device="cuda:0") for _ in range(3)]
    record = [torch.zeros((height, width, 8), dtype=torch.float32, device="cuda:0") for _ in range(3)]
    matrix = ref.matrix_of(pods[0])

    def call(samples_in=16, prev_matrix=matrix, guide=record[0], rgb_in=rgb[0], prev_rgb=rgb[1], prev_record=record[1], out=rgb[2], record_out=record[2], record_offset=0):
        tracer.reproject_device(width, height, prev_matrix, guide.data_ptr(), rgb_in.data_ptr(), samples_in, prev_rgb.data_ptr() if prev_rgb is not None else None, prev_record.data_ptr() if prev_record is not None else None, None,
                                out.data_ptr(), record_out.data_ptr() + record_offset)

    call()  # (the arguments the refusals below are variations of are accepted)
    torch.cuda.synchronize()
    for samples_in in (0, 4097):
        with pytest.raises(rt_amd.RtHipError) as refused:
            call(samples_in=samples_in)
        assert refused.value.status == INVALID_ARGUMENT and "samples_in" in str(refused.value)
    for overlapping in ({"out": rgb[0]}, {"out": rgb[1]}, {"record_out": record[1]}, {"record_out": record[0]}):
        with pytest.raises(rt_amd.RtHipError) as refused:
            call(**overlapping)
        assert refused.value.status == INVALID_ARGUMENT and "overlaps" in str(refused.value), overlapping
    with pytest.raises(rt_amd.RtHipError) as refused:
        call(prev_record=None)
    assert refused.value.status == INVALID_ARGUMENT and "together" in str(refused.value)
    with pytest.raises(rt_amd.RtHipError) as refused:
        call(record_offset=4)
    assert refused.value.status == INVALID_ARGUMENT and "aligned" in str(refused.value)
    singular = matrix.copy().reshape(4, 4)
    singular[3] = singular[2]
    with pytest.raises(rt_amd.RtHipError) as refused:
        call(prev_matrix=singular)
    assert refused.value.status == INVALID_ARGUMENT and "singular" in str(refused.value)
    call(prev_matrix=None, prev_rgb=None, prev_record=None)  # no history: no matrix is needed
    torch.cuda.synchronize()


# ---- the drop-in ------------------------------------------------------------------------------------------------------------------
W, H, SPP = 48, 27, 16
SEEDS = (11, 12, 13, 14)
POSES = [((0.0, 1.0, 3.0), cases.FORWARD), ((0.06, 1.0, 3.0), cases.FORWARD), ((0.12, 1.02, 2.95), cases.FORWARD), ((0.12, 1.02, 2.95), cases.yaw(cases.FORWARD, 3.0))]


def pose_pod(k, spp=SPP, width=W, height=H):
    return cases.toml_scene("basic", width, height, *POSES[k], spp=spp)


@functools.lru_cache(maxsize=None)
def composition(filtered):
    """The four delivered frames as the CPU composes them: [(rgba, rgb, pixels with history)]."""
    frames = []
    for k, seed in enumerate(SEEDS):
        pod = pose_pod(k)
        frames.append((pod, cases.guide_of(pod, W, H), oracle.render(pod, W, H, seed=seed)[1], SPP))
    out = []
    for (pod, guide, _, _), (blended, _, found) in zip(frames, ref.sequence(frames)):
        if filtered:
            rgb, rgba = filter_ref.filter(blended, guide, filter_ref.params())
        else:
            rgb, rgba = blended, filter_ref.finish(blended)
        out.append((rgba, rgb, found))
    return out


@pytest.mark.parametrize("filtered", [False, True], ids=["blended", "blended_and_filtered"])
def test_four_frames_of_a_moving_camera_are_the_composition_packed_and_float(filtered):
    with rt_amd.HipRayTracer(device=0) as tracer:
        for k, seed in enumerate(SEEDS):
            rgba, rgb, stats, info = tracer.render_temporal(pose_pod(k), W, H, seed=seed, filter=filter_ref.params() if filtered else None, want_rgb=True)
            want_rgba, want_rgb, want_found = composition(filtered)[k]
            assert np.array_equal(bits(rgb), bits(want_rgb)), f"frame {k}: {(bits(rgb) != bits(want_rgb)).any(axis=-1).sum()} pixels differ"
            assert np.array_equal(rgba, want_rgba), f"frame {k}"
            assert info == {"frames": k + 1, "restarted": 1 if k == 0 else 0, "pixels_with_history": want_found, "pixels": W * H}
            assert (want_found > 0) == (k > 0)
            assert stats["primary_samples"] == W * H * SPP and stats["render_ms"] > 0.0
        # packed pixels alone, without stats: the same frame again would be another blend — a fifth frame with the fourth's seed and pose
        rgba, rgb, stats, info = tracer.render_temporal(pose_pod(3), W, H, seed=SEEDS[3], want_rgb=False, stats=False)
        assert rgb is None and stats == {} and info["frames"] == 5 and info["restarted"] == 0
    assert not np.array_equal(composition(True)[3][0], composition(False)[3][0])
    assert rt_amd.live_frame_locks() == 0


def test_what_restarts_the_history_and_what_does_not():
    with rt_amd.HipRayTracer(device=0) as tracer:
        def frame(pod, seed, width=W, height=H, flags=0):
            return tracer.render_temporal(pod, width, height, seed=seed, flags=flags)[3]

        spheres = list(cases.SURROUND_SPHERES)
        base = lambda k=0, spp=SPP, s=spheres: cases.box_ref.scene_pod(pose_pod(k), spheres=s, planes=cases.SURROUND_PLANES, spp=spp)  # noqa: E731
        assert frame(base(), 1) == {"frames": 1, "restarted": 1, "pixels_with_history": 0, "pixels": W * H}
        # carried on: another matrix, another seed, another samples_per_pixel, the flags that trace the same frame
        for k, (pod, seed, flags) in enumerate([(base(1), 2, 0), (base(1), 3, 0), (base(1, spp=32), 4, 0), (base(1), 5, capi.RT_HIP_FLAG_BVH | capi.RT_HIP_FLAG_STATS)], start=2):
            info = frame(pod, seed, flags=flags)
            assert info["frames"] == k and info["restarted"] == 0 and info["pixels_with_history"] > 0, info
        # started again: a changed sphere, a changed size, a changed max_bounces, the other scatter table
        moved = [(0.1, 1, 0, 1, 0)] + spheres[1:]
        assert frame(base(1, s=moved), 6) == {"frames": 1, "restarted": 1, "pixels_with_history": 0, "pixels": W * H}
        assert frame(base(1, s=moved), 7)["frames"] == 2
        smaller = cases.box_ref.scene_pod(pose_pod(1, width=W - 1), spheres=moved, planes=cases.SURROUND_PLANES, spp=SPP)
        assert frame(smaller, 8, width=W - 1) == {"frames": 1, "restarted": 1, "pixels_with_history": 0, "pixels": (W - 1) * H}
        assert frame(smaller, 9, width=W - 1)["restarted"] == 0
        fewer_bounces = cases.box_ref.scene_pod(pose_pod(1, width=W - 1), spheres=moved, planes=cases.SURROUND_PLANES, spp=SPP, bounces=3)
        info = frame(fewer_bounces, 10, width=W - 1)
        assert info["restarted"] == 1 and info["pixels_with_history"] == 0 and info["frames"] == 1
        info = frame(fewer_bounces, 11, width=W - 1, flags=capi.RT_HIP_FLAG_SM_MATERIALS)
        assert info["restarted"] == 1 and info["pixels_with_history"] == 0
    assert rt_amd.live_frame_locks() == 0


def test_the_history_leaves_rt_hip_render_and_a_progressive_accumulation_alone():
    one_shot = {spp: oracle.render(pose_pod(0, spp=spp), W, H, seed=5) for spp in (16, 32, 48)}
    with rt_amd.HipRayTracer(device=0) as tracer:
        for k, seed in enumerate(SEEDS):
            tracer.render_temporal(pose_pod(k), W, H, seed=seed, filter=filter_ref.params())
        rgba, rgb, _ = tracer.render(pose_pod(0), W, H, seed=5, want_rgb=True)
        assert np.array_equal(rgba, one_shot[16][0]) and np.array_equal(bits(rgb), bits(one_shot[16][1]))
        # a progressive frame of 48 samples in three passes, a temporal frame of ANOTHER pose between any two of them
        for done in (16, 32, 48):
            rgba, rgb, _, progress = tracer.render_progressive(pose_pod(0, spp=48), W, H, seed=5, pass_samples=16, want_rgb=True)
            assert progress["samples_done"] == done and progress["restarted"] == (1 if done == 16 else 0)
            assert np.array_equal(rgba, one_shot[done][0]) and np.array_equal(bits(rgb), bits(one_shot[done][1])), done
            info = tracer.render_temporal(pose_pod(2), W, H, seed=20 + done, filter=filter_ref.params())[3]
            assert info["restarted"] == 0 and info["frames"] == 4 + done // 16  # ... and the passes leave the history alone
            got = tracer.denoise_progressive(None, want_rgb=True)  # the denoiser's kept guide is still the accumulation's
            want = filter_ref.filter(one_shot[done][1], cases.guide_of(pose_pod(0), W, H), None)
            assert np.array_equal(bits(got[1]), bits(want[0])) and np.array_equal(got[0], want[1])
    assert rt_amd.live_frame_locks() == 0


def test_render_temporals_refusals():
    flags = {"RT_HIP_FLAG_FAST": capi.RT_HIP_FLAG_FAST, "RT_HIP_FLAG_PREVIEW": capi.RT_HIP_FLAG_PREVIEW, "RT_HIP_FLAG_FORCE_TILED": capi.RT_HIP_FLAG_FORCE_TILED, "RT_HIP_FLAG_FORCE_RESIDENT": capi.RT_HIP_FLAG_FORCE_RESIDENT,
             "RT_HIP_FLAG_FORCE_STREAMED": capi.RT_HIP_FLAG_FORCE_STREAMED, "RT_HIP_FLAG_FORCE_HALF_CHUNKS": capi.RT_HIP_FLAG_FORCE_HALF_CHUNKS, "RT_HIP_FLAG_FORCE_WHOLE_CHUNKS": capi.RT_HIP_FLAG_FORCE_WHOLE_CHUNKS,
             "RT_HIP_FLAG_PERSISTENT_FRAME": capi.RT_HIP_FLAG_PERSISTENT_FRAME, "unknown flag bits": 1 << 20}
    with rt_amd.HipRayTracer(device=0) as tracer:
        for name, flag in flags.items():
            with pytest.raises(rt_amd.RtHipError) as refused:
                tracer.render_temporal(pose_pod(0), W, H, seed=1, flags=flag)
            assert refused.value.status == UNSUPPORTED and name in str(refused.value), name
        with pytest.raises(rt_amd.RtHipError) as refused:
            tracer.render_temporal(pose_pod(0, spp=4097), W, H, seed=1)
        assert refused.value.status == INVALID_ARGUMENT and "4097" in str(refused.value)
        # the accepted flags are accepted, together
        accepted = capi.RT_HIP_FLAG_SM_MATERIALS | capi.RT_HIP_FLAG_BVH | capi.RT_HIP_FLAG_BVH_DEVICE_BUILD | capi.RT_HIP_FLAG_TRACE_BOXES | capi.RT_HIP_FLAG_STATS
        assert tracer.render_temporal(pose_pod(0), W, H, seed=1, flags=accepted)[3]["frames"] == 1
    with rt_amd.HipRayTracer(devices=[0], peer_copy=True) as multi:
        with pytest.raises(rt_amd.RtHipError) as refused:
            multi.render_temporal(pose_pod(0), W, H, seed=1)
        assert refused.value.status == UNSUPPORTED and "rt_hip_create" in str(refused.value)
    assert rt_amd.live_frame_locks() == 0


def test_with_traced_boxes_the_drop_in_blends_the_box_frames():
    """boxes.toml under RT_HIP_FLAG_TRACE_BOXES, two frames: the traced frame, the guide and therefore the history see the boxes."""
    pods, guides, _ = cases.case("boxes:dolly", W, H)
    frames = [(pod, guide, cases.box_ref.render(pod, W, H, seed=seed)[1], SPP) for pod, guide, seed in zip(pods, guides, (41, 42))]
    want = ref.sequence(frames)
    with rt_amd.HipRayTracer(device=0) as tracer:
        for k, seed in enumerate((41, 42)):
            rgba, rgb, _, info = tracer.render_temporal(pods[k], W, H, seed=seed, flags=BOXES, want_rgb=True)
            assert np.array_equal(bits(rgb), bits(want[k][0])) and np.array_equal(rgba, filter_ref.finish(want[k][0])) and info["pixels_with_history"] == want[k][2]
    assert rt_amd.live_frame_locks() == 0


# ---- the plug-in and the headless driver ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("denoise", [False, True], ids=["temporal", "temporal_and_denoise"])
def test_rt_headless_writes_the_last_of_three_temporal_frames_as_capi_delivers_it(tmp_path, denoise):
    """--temporal --frames 3 --dolly 0.05,0,0 --seed 7: frames 1, 2, 3 get seeds 8, 9, 10 and the camera steps by 0.05 along x before the
    second and the third."""
    with rt_amd.HipRayTracer(device=0) as tracer:
        for k in range(3):
            pod = cases.toml_scene("basic", W, H, (float(F32(0.05) * F32(k)), 1.0, 3.0), cases.FORWARD, spp=SPP)
            want = tracer.render_temporal(pod, W, H, seed=7 + k + 1, filter=filter_ref.params() if denoise else None)[0]
    binary = ROOT / "rt_amd" / "bin" / "rt_headless"
    out = tmp_path / "frame.ppm"
    env = dict(os.environ)
    for name in ("RT_HIP_PROGRESSIVE", "RT_HIP_DENOISE", "RT_HIP_TEMPORAL", "RT_HIP_SEED"):
        env.pop(name, None)
    command = [str(binary), "--renderer", "hip", "--scene", "basic.toml", "--temporal", "--frames", "3", "--dolly", "0.05,0,0", "--seed", "7", "--size", f"{W}x{H}", "--spp", str(SPP), *(["--denoise"] if denoise else []), "--out", str(out)]
    done = subprocess.run(command, cwd=ROOT, capture_output=True, text=True, timeout=300, env=env)
    assert done.returncode == 0 and "error" not in done.stderr, done.stderr
    header = f"P6\n{W} {H}\n255\n".encode()
    data = out.read_bytes()
    assert data.startswith(header)
    assert np.array_equal(np.frombuffer(data[len(header):], dtype=np.uint8).reshape(H, W, 3), unpack(want)[..., :3])


def test_on_a_multi_gpu_plug_in_temporal_is_refused_once_and_whole_frames_are_rendered(tmp_path):
    """RT_HIP_DEVICES=0 makes the plug-in's context a multi-GPU one, which rt_hip_render_temporal refuses: one error line, and every
    frame is rt_hip_render's with the seed the temporal frame would have had (7 + 2 for the second)."""
    binary = ROOT / "rt_amd" / "bin" / "rt_headless"
    out = tmp_path / "frame.ppm"
    env = dict(os.environ, RT_HIP_DEVICES="0")
    for name in ("RT_HIP_PROGRESSIVE", "RT_HIP_DENOISE", "RT_HIP_TEMPORAL", "RT_HIP_SEED", "RT_HIP_GROUP"):
        env.pop(name, None)
    command = [str(binary), "--renderer", "hip", "--scene", "basic.toml", "--temporal", "--frames", "2", "--seed", "7", "--size", f"{W}x{H}", "--spp", str(SPP), "--out", str(out)]
    done = subprocess.run(command, cwd=ROOT, capture_output=True, text=True, timeout=300, env=env)
    assert done.returncode == 0, done.stderr
    assert done.stderr.count("RT_HIP_TEMPORAL is ignored") == 1 and done.stderr.count("error:") == 1, done.stderr
    want = oracle.render(cases.toml_scene("basic", W, H, spp=SPP), W, H, seed=9)[0]
    header = f"P6\n{W} {H}\n255\n".encode()
    data = out.read_bytes()
    assert data.startswith(header)
    assert np.array_equal(np.frombuffer(data[len(header):], dtype=np.uint8).reshape(H, W, 3), unpack(want)[..., :3])
