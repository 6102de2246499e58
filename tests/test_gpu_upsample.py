"""Guided upsampling on the GPU, tolerance 0 throughout: the reconstruction (rt_hip_upsample_device) against the serial
CPU restatement over the kernel's own per-pixel text (tests/upsample_reference.py) — the bit patterns of d_rgb_out, the words of
d_rgba8_out and the orphan count — and the drop-in (rt_hip_render_upscaled) against the composition built here from the device-level
calls it stands for: rt_hip_render_device at the low size, rt_hip_guide_device twice, then the restatement."""
import functools
import os
import subprocess
import uuid

import numpy as np
import pytest

import rt_amd
from rt_amd import capi
from tests import denoise_reference as denoise_ref
from tests import upsample_reference as ref
from tests.conftest import GOLDEN, ROOT, unpack

pytestmark = pytest.mark.gpu

F32 = np.float32
W, H = 96, 54
SEED = 5
BOXES = capi.RT_HIP_FLAG_TRACE_BOXES
TILTED = ((0.2, 1.2, 3.0), (0.0, -0.15, -1.0))
INVALID_ARGUMENT, UNSUPPORTED = 1, 5
LOW = {2: (48, 27), 3: (32, 18), 4: (24, 14)}  # (54 / 4 is ragged)


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def basic(spp=16, tilted=False):
    """basic.toml with the matrix of the FULL frame: the low frame is traced through the same one."""
    scene = rt_amd.Scene.named("basic").set_sampling(spp)
    if tilted:
        scene.set_camera(*TILTED)
    return scene.describe(W, H)


def boxes_toml():
    return rt_amd.Scene.load(GOLDEN / "scenes" / "boxes.toml").set_sampling(16).describe(W, H)


SCENES = {"basic": (basic, 0), "basic_tilted": (lambda: basic(tilted=True), 0), "boxes": (boxes_toml, BOXES)}


def stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def traced_inputs(tracer, pod, flags, w, h, seed=SEED):
    """What the drop-in makes on its way, by the device-level calls: the low float mean, the low guide and the full guide."""
    import torch

    device = f"cuda:{tracer.device}"
    tracer.upload(pod)
    d_rgba = torch.zeros((h, w), dtype=torch.int32, device=device)
    d_rgb = torch.full((h, w, 3), float("nan"), dtype=torch.float32, device=device)
    tracer.render_device(w, h, d_rgba.data_ptr(), seed=seed, flags=flags, d_rgb_f32=d_rgb.data_ptr(), stream=stream())
    d_low = torch.full((h, w, 8), float("nan"), dtype=torch.float32, device=device)
    d_full = torch.full((H, W, 8), float("nan"), dtype=torch.float32, device=device)
    tracer.guide_device(w, h, d_low.data_ptr(), flags=flags & BOXES, stream=stream())
    tracer.guide_device(W, H, d_full.data_ptr(), flags=flags & BOXES, stream=stream())
    return d_rgb.cpu().numpy(), d_low.cpu().numpy(), d_full.cpu().numpy()


_inputs = {}


def inputs(tracer, scene, factor):
    """Computed once per case and shared, read-only."""
    key = (scene, factor)
    if key not in _inputs:
        make, flags = SCENES[scene]
        arrays = traced_inputs(tracer, make(), flags, *LOW[factor])
        for a in arrays:
            a.setflags(write=False)
        _inputs[key] = arrays
    return _inputs[key]


def device_upsample(tracer, low, guide_low, guide_full, p, want_rgb=True, want_rgba=True, want_orphans=True):
    import torch

    device = f"cuda:{tracer.device}"
    h, w = low.shape[:2]
    height, width = guide_full.shape[:2]
    d_low = torch.from_numpy(np.array(low, dtype=F32)).to(device)  # (np.array: a copy, the cached arrays are read-only)
    d_guide_low = torch.from_numpy(np.array(guide_low, dtype=F32)).to(device)
    d_guide_full = torch.from_numpy(np.array(guide_full, dtype=F32)).to(device)
    d_out = torch.full((height, width, 3), float("nan"), dtype=torch.float32, device=device) if want_rgb else None
    d_rgba = torch.zeros((height, width), dtype=torch.int32, device=device) if want_rgba else None
    d_orphans = torch.full((1,), 12345, dtype=torch.int32, device=device) if want_orphans else None  # (overwritten, not added to)
    tracer.upsample_device(width, height, w, h, d_low.data_ptr(), d_guide_low.data_ptr(), d_guide_full.data_ptr(), p, d_out.data_ptr() if want_rgb else None, d_rgba.data_ptr() if want_rgba else None,
                           d_orphans.data_ptr() if want_orphans else None, stream=stream())
    assert np.array_equal(bits(d_low.cpu().numpy()), bits(low))  # (the inputs are not touched)
    return (d_out.cpu().numpy() if want_rgb else None), (d_rgba.cpu().numpy().view(np.uint32) if want_rgba else None), (int(d_orphans.cpu().numpy()[0]) if want_orphans else None)


def assert_is_the_restatement(tracer, low, guide_low, guide_full, p, what):
    got_rgb, got_rgba, got_orphans = device_upsample(tracer, low, guide_low, guide_full, p)
    want_rgb, want_rgba, want_orphans = ref.frame(low, guide_low, guide_full, p)
    differing = (bits(got_rgb) != bits(want_rgb)).any(axis=-1)
    assert not differing.any(), f"{what}: {differing.sum()} of {differing.size} pixels differ from the restatement, first at (y, x) = {tuple(np.argwhere(differing)[0])}"
    assert np.array_equal(got_rgba, want_rgba), what
    assert got_orphans == want_orphans, what
    return want_orphans


# ---- the device entry -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["basic", "boxes"])
@pytest.mark.parametrize("factor", [2, 3, 4])
def test_a_real_16_spp_mean_and_real_guides(tracer, scene, factor):
    low, guide_low, guide_full = inputs(tracer, scene, factor)
    assert low.shape[:2] == LOW[factor][::-1] and np.isfinite(low).all()
    ids = guide_full[..., 7].copy().view(np.uint32)
    assert (ids == 0).any() and (ids != 0).any()  # sky and surfaces: both kinds of edge
    if scene == "boxes":
        pod = boxes_toml()
        assert (ids > pod.n_spheres + pod.n_planes).any()  # the flag made the guides see the boxes
    orphans = assert_is_the_restatement(tracer, low, guide_low, guide_full, ref.params(), f"{scene} / {factor}")
    assert orphans < W * H // 4  # (most of the frame found its surface among its taps)
    # tight and wide terms, a threshold that makes many orphans
    assert_is_the_restatement(tracer, low, guide_low, guide_full, ref.params(normal_squarings=8, sigma_albedo=0.01, sigma_depth=0.001, min_weight=0.5), f"{scene} / {factor}, tight")
    assert_is_the_restatement(tracer, low, guide_low, guide_full, ref.params(normal_squarings=0, sigma_albedo=10.0, sigma_depth=10.0, min_weight=1e-6), f"{scene} / {factor}, wide")


# 1 x 1; one low pixel under a block; one pixel past a workgroup corner; w == W (the widest staging span); one low column under three
# workgroups; no whole ratio, several blocks each way
SHAPES = [(1, 1, 1, 1), (2, 2, 1, 1), (17, 17, 9, 9), (33, 5, 33, 5), (37, 3, 1, 1), (70, 41, 18, 11)]


@pytest.mark.parametrize("width,height,w,h", SHAPES)
def test_random_guides_and_colours_with_a_nan_and_an_inf_low_pixel(tracer, width, height, w, h):
    rng = np.random.default_rng(1000 * width + w)
    low = rng.uniform(-0.2, 1.5, size=(h, w, 3)).astype(F32)
    guide_low, guide_full = ref.random_guide(rng, h, w), ref.random_guide(rng, height, width)
    what = f"{width}x{height} from {w}x{h}"
    assert_is_the_restatement(tracer, low, guide_low, guide_full, ref.params(sigma_albedo=0.5, sigma_depth=0.5), what)
    low[h // 2, w // 3, 1] = np.nan
    low[h - 1, w - 1, 2] = np.inf
    for p in (ref.params(sigma_albedo=0.5, sigma_depth=0.5), ref.params(normal_squarings=0, sigma_albedo=5.0, sigma_depth=5.0, min_weight=1.0)):
        assert_is_the_restatement(tracer, low, guide_low, guide_full, p, what + ", poisoned")
    # one surface everywhere: the plain bilinear frame, nobody an orphan
    low = rng.uniform(0.0, 1.0, size=(h, w, 3)).astype(F32)
    assert assert_is_the_restatement(tracer, low, ref.hit_guide(h, w), ref.hit_guide(height, width), None, what + ", one surface") == 0


def test_either_output_alone_both_and_no_orphan_word(tracer):
    low, guide_low, guide_full = inputs(tracer, "basic", 3)
    want_rgb, want_rgba, want_orphans = ref.frame(low, guide_low, guide_full)
    got = device_upsample(tracer, low, guide_low, guide_full, None, want_rgba=False)
    assert np.array_equal(bits(got[0]), bits(want_rgb)) and got[1] is None and got[2] == want_orphans
    got = device_upsample(tracer, low, guide_low, guide_full, None, want_rgb=False)
    assert got[0] is None and np.array_equal(got[1], want_rgba) and got[2] == want_orphans
    got = device_upsample(tracer, low, guide_low, guide_full, None, want_orphans=False)
    assert np.array_equal(bits(got[0]), bits(want_rgb)) and np.array_equal(got[1], want_rgba) and got[2] is None


def test_a_null_params_is_the_defaults(tracer):
    low, guide_low, guide_full = inputs(tracer, "basic", 2)
    by_null = device_upsample(tracer, low, guide_low, guide_full, None)
    by_defaults = device_upsample(tracer, low, guide_low, guide_full, rt_amd.renderer.upsample_default_params())
    want = ref.frame(low, guide_low, guide_full, ref.params())
    for got in (by_null, by_defaults):
        assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[1], want[1]) and got[2] == want[2]
    other = device_upsample(tracer, low, guide_low, guide_full, ref.params(sigma_depth=5.0))
    assert not np.array_equal(bits(other[0]), bits(want[0]))  # (the parameters matter)


def test_the_device_entrys_refusals(tracer):
    import torch

    low = torch.zeros((27, 48, 3), dtype=torch.float32, device="cuda:0")
    guide_low = torch.zeros((27, 48, 8), dtype=torch.float32, device="cuda:0")
    guide_full = torch.zeros((H, W, 8), dtype=torch.float32, device="cuda:0")
    out = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda:0")
    rgba = torch.zeros((H, W), dtype=torch.int32, device="cuda:0")
    word = torch.zeros((4,), dtype=torch.int32, device="cuda:0")
    args = dict(width=W, height=H, low_width=48, low_height=27, d_rgb_low=low.data_ptr(), d_guide_low=guide_low.data_ptr(), d_guide_full=guide_full.data_ptr(), params=None, d_rgb_out=out.data_ptr(), d_rgba8_out=rgba.data_ptr(),
                d_orphans=word.data_ptr())
    tracer.upsample_device(**args)  # (as it stands it is accepted)
    cases = [
        (dict(d_rgb_out=None, d_rgba8_out=None), "both NULL"),
        (dict(d_rgb_low=None), "NULL"),
        (dict(d_guide_low=None), "NULL"),
        (dict(d_guide_full=None), "NULL"),
        (dict(width=0), "full frame"),
        (dict(height=(1 << 22) + 1), "full frame"),
        (dict(low_width=0), "low frame"),
        (dict(low_width=W + 1), "low frame"),
        (dict(low_height=H + 1), "low frame"),
        (dict(d_guide_low=guide_low.data_ptr() + 4), "aligned"),
        (dict(d_guide_full=guide_full.data_ptr() + 8), "aligned"),
        (dict(d_rgb_out=low.data_ptr()), "d_rgb_out overlaps d_rgb_low"),
        (dict(d_rgba8_out=guide_full.data_ptr() + 16 * W), "d_rgba8_out overlaps d_guide_full"),
        (dict(d_orphans=guide_low.data_ptr() + 64), "d_orphans overlaps d_guide_low"),
        (dict(d_rgba8_out=out.data_ptr() + 12), "d_rgb_out overlaps d_rgba8_out"),
        (dict(d_orphans=rgba.data_ptr() + 4 * (W * H - 1)), "d_rgba8_out overlaps d_orphans"),
        (dict(params=ref.params(min_weight=0.0)), "min_weight"),
        (dict(params=ref.params(normal_squarings=9)), "normal_squarings"),
        (dict(params=ref.params(sigma_albedo=float("nan"))), "sigma_albedo"),
        (dict(params=ref.params(sigma_depth=-1.0)), "sigma_depth"),
    ]
    for changed, named in cases:
        with pytest.raises(rt_amd.RtHipError) as refused:
            tracer.upsample_device(**dict(args, **changed))
        assert refused.value.status == INVALID_ARGUMENT and named in str(refused.value), (changed, str(refused.value))


def test_on_a_multi_context_the_root_member_answers(tracer):
    low, guide_low, guide_full = inputs(tracer, "basic", 4)
    with rt_amd.HipRayTracer(devices=[0], peer_copy=True) as multi:
        assert_is_the_restatement(multi, low, guide_low, guide_full, None, "multi")


# ---- the drop-in ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("factor", [2, 4])
@pytest.mark.parametrize("filtered", [False, True])
def test_render_upscaled_is_the_composition_of_the_device_level_calls(tracer, factor, filtered):
    w, h = LOW[factor]
    low, guide_low, guide_full = inputs(tracer, "basic", factor)
    filter_params = denoise_ref.params(iterations=2, normal_squarings=5, sigma_colour=0.6, sigma_albedo=0.1, sigma_depth=0.05) if filtered else None
    low_in = denoise_ref.filter(low, guide_low, filter_params)[0] if filtered else low
    p = ref.params(sigma_depth=0.05)
    want_rgb, want_rgba, want_orphans = ref.frame(low_in, guide_low, guide_full, p)
    with rt_amd.HipRayTracer(device=0) as fresh:
        rgba, rgb, stats, info = fresh.render_upscaled(basic(16), W, H, seed=SEED, factor=factor, upsample=p, filter=filter_params, want_rgb=True)
        assert np.array_equal(bits(rgb), bits(want_rgb)) and np.array_equal(rgba, want_rgba)
        assert info == {"low_width": w, "low_height": h, "orphans": want_orphans, "pixels": W * H}
        assert stats["primary_samples"] == w * h * 16 and stats["render_ms"] > 0.0
        # again (the scratch is kept), the packed frame alone, without stats
        rgba, rgb, stats, info = fresh.render_upscaled(basic(16), W, H, seed=SEED, factor=factor, upsample=p, filter=filter_params, stats=False)
        assert np.array_equal(rgba, want_rgba) and rgb is None and stats == {} and info["orphans"] == want_orphans
    assert (rt_amd.renderer.upsample_low_size(W, H, factor)) == (w, h)


def test_the_defaults_the_boxes_flag_and_the_flags_that_change_nothing(tracer):
    low, guide_low, guide_full = inputs(tracer, "boxes", 3)
    want_rgb, want_rgba, want_orphans = ref.frame(low, guide_low, guide_full)
    same = capi.RT_HIP_FLAG_BVH | capi.RT_HIP_FLAG_BVH_DEVICE_BUILD | capi.RT_HIP_FLAG_STATS
    for flags in (BOXES, BOXES | same):
        rgba, rgb, _, info = tracer.render_upscaled(boxes_toml(), W, H, seed=SEED, flags=flags, factor=3, want_rgb=True)
        assert np.array_equal(bits(rgb), bits(want_rgb)) and np.array_equal(rgba, want_rgba) and info["orphans"] == want_orphans


def test_a_call_leaves_a_progressive_accumulation_in_flight_untouched(tracer):
    one_shot = {spp: tracer.render(basic(spp), W, H, seed=SEED, want_rgb=True)[:2] for spp in (16, 32)}
    with rt_amd.HipRayTracer(device=0) as fresh:
        rgba, rgb, _, progress = fresh.render_progressive(basic(48), W, H, seed=SEED, pass_samples=16, want_rgb=True)
        assert progress["samples_done"] == 16 and np.array_equal(rgba, one_shot[16][0]) and np.array_equal(bits(rgb), bits(one_shot[16][1]))
        low, guide_low, guide_full = inputs(tracer, "basic_tilted", 2)  # another matrix ...
        low_seed9 = traced_inputs(tracer, basic(tilted=True), 0, *LOW[2], seed=9)[0]  # ... and another seed
        assert not np.array_equal(bits(low_seed9), bits(low))
        want = ref.frame(low_seed9, guide_low, guide_full)
        for _ in range(2):
            got_rgba, got_rgb, _, info = fresh.render_upscaled(basic(tilted=True), W, H, seed=9, factor=2, want_rgb=True)
            assert np.array_equal(bits(got_rgb), bits(want[0])) and np.array_equal(got_rgba, want[1]) and info["orphans"] == want[2]
        rgba, rgb, _, progress = fresh.render_progressive(basic(48), W, H, seed=SEED, pass_samples=16, want_rgb=True)
        assert progress["samples_done"] == 32 and progress["restarted"] == 0
        assert np.array_equal(rgba, one_shot[32][0]) and np.array_equal(bits(rgb), bits(one_shot[32][1]))
    assert rt_amd.live_frame_locks() == 0


def test_the_drop_ins_refusals(tracer):
    refused_flags = [(capi.RT_HIP_FLAG_FAST, "RT_HIP_FLAG_FAST"), (capi.RT_HIP_FLAG_PREVIEW, "RT_HIP_FLAG_PREVIEW"), (capi.RT_HIP_FLAG_FORCE_TILED, "RT_HIP_FLAG_FORCE_TILED"),
                     (capi.RT_HIP_FLAG_FORCE_RESIDENT, "RT_HIP_FLAG_FORCE_RESIDENT"), (capi.RT_HIP_FLAG_FORCE_STREAMED, "RT_HIP_FLAG_FORCE_STREAMED"), (capi.RT_HIP_FLAG_FORCE_HALF_CHUNKS, "RT_HIP_FLAG_FORCE_HALF_CHUNKS"),
                     (capi.RT_HIP_FLAG_FORCE_WHOLE_CHUNKS, "RT_HIP_FLAG_FORCE_WHOLE_CHUNKS"), (capi.RT_HIP_FLAG_PERSISTENT_FRAME, "RT_HIP_FLAG_PERSISTENT_FRAME"), (BOXES | capi.RT_HIP_FLAG_BOX_BVH, "RT_HIP_FLAG_BOX_BVH"),
                     (capi.RT_HIP_FLAG_EMISSION, "RT_HIP_FLAG_EMISSION"), (capi.RT_HIP_FLAG_EMISSION | capi.RT_HIP_FLAG_DIRECT_LIGHT, "RT_HIP_FLAG_EMISSION"), (1 << 20, "unknown flag bits")]
    for flags, named in refused_flags:
        with pytest.raises(rt_amd.RtHipError) as refused:
            tracer.render_upscaled(basic(), W, H, seed=1, flags=flags)
        assert refused.value.status == UNSUPPORTED and named in str(refused.value) and "rt_hip_render_upscaled" in str(refused.value)
    for factor in (0, 1, 5):
        with pytest.raises(rt_amd.RtHipError) as refused:
            tracer.render_upscaled(basic(), W, H, seed=1, factor=factor)
        assert refused.value.status == INVALID_ARGUMENT and "factor" in str(refused.value)
    with pytest.raises(rt_amd.RtHipError) as refused:
        tracer.render_upscaled(basic(), (1 << 15) + 1, H, seed=1)
    assert refused.value.status == INVALID_ARGUMENT and "frame" in str(refused.value)


def test_multi_rank_and_group_contexts_are_unsupported():
    with rt_amd.HipRayTracer(devices=[0], peer_copy=True) as multi:
        with pytest.raises(rt_amd.RtHipError) as refused:
            multi.render_upscaled(basic(), W, H, seed=1)
        assert refused.value.status == UNSUPPORTED and "rt_hip_create" in str(refused.value)
    with rt_amd.HipRayTracer(device=0, rank=0, world=1, unique_id=rt_amd.unique_id()) as rank:
        with pytest.raises(rt_amd.RtHipError) as refused:
            rank.render_upscaled(basic(), W, H, seed=1)
        assert refused.value.status == UNSUPPORTED and "rt_hip_create" in str(refused.value)
    with rt_amd.HipRayTracer(device=0) as member:
        member.join_frame_group(0, 1, f"/rt_hip_test_{uuid.uuid4().hex[:12]}", timeout_ms=5000)
        with pytest.raises(rt_amd.RtHipError) as refused:
            member.render_upscaled(basic(), W, H, seed=1)
        assert refused.value.status == UNSUPPORTED and "rt_hip_create" in str(refused.value)
    assert rt_amd.live_frame_locks() == 0


def test_the_plug_in_and_rt_headless_deliver_the_drop_ins_frame(tracer, tmp_path):
    """RT_HIP_UPSCALE=2 in the plug-in's environment, and rt_headless --upscale 2, which sets it: the file is rt_hip_render_upscaled's
    frame at the defaults; with --denoise the low frame went through the default filter first."""
    binary = ROOT / "rt_amd" / "bin" / "rt_headless"
    common = [str(binary), "--renderer", "hip", "--scene", "basic.toml", "--size", f"{W}x{H}", "--spp", "16"]
    env = dict(os.environ, RT_HIP_SEED=str(SEED))
    for name in ("RT_HIP_PROGRESSIVE", "RT_HIP_DENOISE", "RT_HIP_TEMPORAL", "RT_HIP_ADAPTIVE", "RT_HIP_UPSCALE", "RT_HIP_LIGHTS"):
        env.pop(name, None)
    want_plain = unpack(tracer.render_upscaled(basic(16), W, H, seed=SEED, factor=2)[0])[..., :3]
    want_filtered = unpack(tracer.render_upscaled(basic(16), W, H, seed=SEED, factor=2, filter=rt_amd.renderer.denoise_default_params())[0])[..., :3]
    low, guide_low, guide_full = inputs(tracer, "basic", 2)
    assert np.array_equal(want_plain, unpack(ref.frame(low, guide_low, guide_full)[1])[..., :3])
    assert not np.array_equal(want_plain, want_filtered)
    whole = unpack(tracer.render(basic(16), W, H, seed=SEED)[0])[..., :3]
    assert not np.array_equal(want_plain, whole)  # (a rebuilt frame is not the traced one)
    header = f"P6\n{W} {H}\n255\n".encode()
    for i, (extra, extra_env, want) in enumerate(((["--upscale", "2"], {}, want_plain), ([], {"RT_HIP_UPSCALE": "2"}, want_plain), (["--upscale", "2", "--denoise"], {}, want_filtered), ([], {}, whole))):
        out = tmp_path / f"frame{i}.ppm"
        done = subprocess.run([*common, *extra, "--out", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=300, env=dict(env, **extra_env))
        assert done.returncode == 0 and "error" not in done.stderr, done.stderr
        data = out.read_bytes()
        assert data.startswith(header)
        assert np.array_equal(np.frombuffer(data[len(header) :], dtype=np.uint8).reshape(H, W, 3), want), (extra, extra_env)
