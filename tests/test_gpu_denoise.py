"""The guide-buffer denoiser on the GPU, tolerance 0 throughout: the guide (rt_hip_guide_device) against its oracle
composition, all 8 words; the filter (rt_hip_denoise_device) against the serial CPU restatement over the kernels' own per-pixel text
(tests/denoise_reference.py); and the drop-in (rt_hip_denoise_progressive) on an accumulation in flight, which it must leave alone.
Frames are 37 x 23: ragged against the guide kernel's 64 x 4 blocks and the filter's 32 x 8 tiles, more than one block of each."""
import functools
import os
import subprocess

import numpy as np
import pytest

import rt_amd
from oracle import binding as oracle
from rt_amd import capi
from tests import box_reference as box_ref
from tests import denoise_reference as ref
from tests.conftest import GOLDEN, ROOT, unpack

pytestmark = pytest.mark.gpu

F32 = np.float32
W, H = 37, 23
SEED = 5
BOXES = capi.RT_HIP_FLAG_TRACE_BOXES
TILTED = ((0.2, 1.2, 3.0), (0.0, -0.15, -1.0))
INVALID_ARGUMENT, NO_SCENE, UNSUPPORTED = 1, 4, 5


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def basic(spp=16, tilted=False, width=W, height=H):
    scene = rt_amd.Scene.named("basic").set_sampling(spp)
    if tilted:
        scene.set_camera(*TILTED)
    return scene.describe(width, height)


def planes_only(width=W, height=H):
    """A floor and a slope that rises to the left, nothing else: the upper right of the frame is sky."""
    return box_ref.scene_pod(basic(width=width, height=height), planes=[(0, 1, 0, 0, 0), (0.6, 0.8, 0, 2, 3)])


def orthographic(width=W, height=H):
    """basic's primitives through a matrix without a finite eye (last row 0 0 0 1): the homogeneous form of the primary ray."""
    pod = box_ref.scene_pod(basic(width=width, height=height), spheres=[(0, 1, 0, 1, 0), (2, 0.5, -1, 0.5, 1), (-1.5, 0.4, 1, 0.4, 3)], planes=[(0, 1, 0, 0, 0)])
    matrix = np.array([[4, 0, 0, 0.25], [0, 2.25, 0.5, 1.5], [0, 0, -10, 5], [0, 0, 0, 1]], dtype=F32)
    for i, v in enumerate(matrix.reshape(-1)):
        pod.inverse_view_projection[i] = float(v)
    return pod


def boxes_toml(width=W, height=H):
    return rt_amd.Scene.load(GOLDEN / "scenes" / "boxes.toml").describe(width, height)


def device_guide(tracer, pod, width, height, flags=0):
    import torch

    tracer.upload(pod)
    guide = torch.full((height, width, 8), float("nan"), dtype=torch.float32, device=f"cuda:{tracer.device}")
    tracer.guide_device(width, height, guide.data_ptr(), flags=flags, stream=torch.cuda.current_stream().cuda_stream)
    return guide.cpu().numpy()


def device_filter(tracer, image, guide, p, want_rgb=True, want_rgba=True):
    import torch

    height, width = image.shape[:2]
    device = f"cuda:{tracer.device}"
    d_in = torch.from_numpy(np.array(image, dtype=F32)).to(device)  # (np.array: a copy, the cached references are read-only)
    d_guide = torch.from_numpy(np.array(guide, dtype=F32)).to(device)
    d_out = torch.full((height, width, 3), float("nan"), dtype=torch.float32, device=device) if want_rgb else None
    d_rgba = torch.zeros((height, width), dtype=torch.int32, device=device) if want_rgba else None
    tracer.denoise_device(width, height, d_in.data_ptr(), d_guide.data_ptr(), p, d_out.data_ptr() if want_rgb else None, d_rgba.data_ptr() if want_rgba else None, stream=torch.cuda.current_stream().cuda_stream)
    assert np.array_equal(bits(d_in.cpu().numpy()), bits(image))  # (the input is not touched)
    return (d_out.cpu().numpy() if want_rgb else None), (d_rgba.cpu().numpy().view(np.uint32) if want_rgba else None)


def assert_filter_is_the_restatement(tracer, image, guide, p, what):
    got_rgb, got_rgba = device_filter(tracer, image, guide, p)
    want_rgb, want_rgba = ref.filter(image, guide, p)
    differing = (bits(got_rgb) != bits(want_rgb)).any(axis=-1)
    assert not differing.any(), f"{what}: {differing.sum()} of {differing.size} pixels differ from the restatement, first at (y, x) = {tuple(np.argwhere(differing)[0])}"
    assert np.array_equal(got_rgba, want_rgba), what


# ---- the guide ------------------------------------------------------------------------------------------------------------------
GUIDE_CASES = {
    "basic_pinhole": (lambda: basic(), W, H, 0, False, "pinhole"),
    "basic_tilted_eye": (lambda: basic(tilted=True), W, H, 0, False, "eye"),
    "orthographic_general": (lambda: orthographic(), W, H, 0, False, "general"),
    "planes_and_sky": (lambda: planes_only(), W, H, 0, False, "pinhole"),
    "boxes_toml_without_the_flag": (lambda: boxes_toml(), W, H, 0, False, None),
    "boxes_toml_with_the_flag": (lambda: boxes_toml(), W, H, BOXES, True, None),
    "one_pixel": (lambda: basic(tilted=True, width=1, height=1), 1, 1, 0, False, None),
}


@functools.lru_cache(maxsize=None)
def composed(name):
    make, width, height, _, boxes, _ = GUIDE_CASES[name]
    guide = ref.compose_guide(make(), width, height, boxes=boxes)
    guide.setflags(write=False)
    return guide


@pytest.mark.parametrize("name", list(GUIDE_CASES))
def test_the_guide_is_the_oracle_composition_in_all_8_words(tracer, name):
    make, width, height, flags, _, form = GUIDE_CASES[name]
    pod = make()
    if form is not None:
        assert oracle.primary_ray(pod, width, height, 0, 0, want_form=True)[2] == form
    want = composed(name)
    ids = want[..., 7].copy().view(np.uint32)
    if name == "planes_and_sky":
        assert (ids == 0).any() and (ids != 0).any()
    if name.startswith("boxes_toml"):
        is_box = ids > pod.n_spheres + pod.n_planes
        assert is_box.any() == bool(flags & BOXES)  # the boxes are in the frame, and only the flag makes the ray hit them
    # the flags that change nothing are accepted and change nothing
    for same in (0, capi.RT_HIP_FLAG_SM_MATERIALS | capi.RT_HIP_FLAG_BVH | capi.RT_HIP_FLAG_BVH_DEVICE_BUILD | capi.RT_HIP_FLAG_STATS):
        got = device_guide(tracer, pod, width, height, flags | same)
        differing = (bits(got) != bits(want)).any(axis=-1)
        assert not differing.any(), f"{name}: {differing.sum()} of {differing.size} pixels differ, first at (y, x) = {tuple(np.argwhere(differing)[0])}: {got[tuple(np.argwhere(differing)[0])]} for {want[tuple(np.argwhere(differing)[0])]}"


def test_the_guides_refusals(tracer):
    import torch

    guide = torch.zeros((H, W, 8), dtype=torch.float32, device="cuda:0")
    tracer.upload(basic())
    for flags, named in ((1 << 20, "unknown flag bits"), (capi.RT_HIP_FLAG_FAST, "RT_HIP_FLAG_FAST"), (capi.RT_HIP_FLAG_PREVIEW, "RT_HIP_FLAG_PREVIEW")):
        with pytest.raises(rt_amd.RtHipError) as refused:
            tracer.guide_device(W, H, guide.data_ptr(), flags=flags)
        assert refused.value.status == UNSUPPORTED and named in str(refused.value)
    with pytest.raises(rt_amd.RtHipError) as refused:
        tracer.guide_device(W, H, guide.data_ptr() + 4)
    assert refused.value.status == INVALID_ARGUMENT and "aligned" in str(refused.value)
    # more boxes than the flag traces: refused with the flag's name, and only with the flag
    many = box_ref.scene_pod(basic(), boxes=[(0.01 * i, 0.5, 0, 0.004, 0.5, 0.5, 0) for i in range(257)])
    tracer.upload(many)
    with pytest.raises(rt_amd.RtHipError) as refused:
        tracer.guide_device(W, H, guide.data_ptr(), flags=BOXES)
    assert refused.value.status == UNSUPPORTED and "RT_HIP_FLAG_TRACE_BOXES" in str(refused.value)
    tracer.guide_device(W, H, guide.data_ptr())
    with rt_amd.HipRayTracer(device=0) as fresh:
        with pytest.raises(rt_amd.RtHipError) as refused:
            fresh.guide_device(W, H, guide.data_ptr())
        assert refused.value.status == NO_SCENE


def test_on_a_multi_context_the_root_member_answers():
    with rt_amd.HipRayTracer(devices=[0], peer_copy=True) as multi:
        got = device_guide(multi, basic(), W, H)
    assert np.array_equal(bits(got), bits(composed("basic_pinhole")))


# ---- the filter -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def noisy_basic():
    """The real 16-spp float mean of basic at 37 x 23 (the oracle's: the device's own frame equals it bit for bit, tests/test_gpu_parity.py)."""
    rgba, rgb, _ = oracle.render(basic(16), W, H, seed=SEED)
    rgb.setflags(write=False), rgba.setflags(write=False)
    return rgb, rgba


@pytest.mark.parametrize("iterations", range(1, 7))
def test_real_guide_and_real_16_spp_mean(tracer, iterations):
    """Iterations 1 and 2 run the LDS-tiled builds, 3 to 6 add the gathering one with steps 4 to 32 (32 is nearly the frame)."""
    p = ref.params(iterations=iterations, normal_squarings=5, sigma_colour=0.6, sigma_albedo=0.1, sigma_depth=0.05)
    assert_filter_is_the_restatement(tracer, noisy_basic()[0], composed("basic_pinhole"), p, f"{iterations} iterations")


def test_the_defaults_and_a_null_params(tracer):
    got_rgb, got_rgba = device_filter(tracer, noisy_basic()[0], composed("basic_pinhole"), None)
    want_rgb, want_rgba = ref.filter(noisy_basic()[0], composed("basic_pinhole"), ref.params())
    assert np.array_equal(bits(got_rgb), bits(want_rgb)) and np.array_equal(got_rgba, want_rgba)
    assert not np.array_equal(bits(got_rgb), bits(noisy_basic()[0]))  # (the defaults filter)


@pytest.mark.parametrize("guide_name", ["basic_pinhole", "planes_and_sky", "boxes_toml_with_the_flag"])
def test_random_images_with_a_nan_and_an_inf_pixel(tracer, guide_name):
    rng = np.random.default_rng(21)
    image = rng.uniform(-0.2, 1.5, size=(H, W, 3)).astype(F32)
    image[7, 30, 0] = np.nan
    image[15, 3, 2] = np.inf
    for iterations, squarings in ((2, 0), (4, 8), (6, 3)):
        p = ref.params(iterations=iterations, normal_squarings=squarings, sigma_colour=1.5, sigma_albedo=0.5, sigma_depth=0.2)
        assert_filter_is_the_restatement(tracer, image, composed(guide_name), p, f"{guide_name}, {iterations} iterations")


@pytest.mark.parametrize("width,height", [(1, 1), (5, 3)])
def test_frames_smaller_than_the_footprint(tracer, width, height):
    rng = np.random.default_rng(22)
    guide = ref.compose_guide(basic(width=width, height=height), width, height)
    image = rng.uniform(0.0, 1.0, size=(height, width, 3)).astype(F32)
    for iterations in (1, 2, 3, 6):
        assert_filter_is_the_restatement(tracer, image, guide, ref.params(iterations=iterations, sigma_colour=2.0, sigma_depth=0.5), f"{width}x{height}, {iterations} iterations")


def test_70_by_41_with_5_iterations(tracer):
    """The step-16 taps (32 pixels out) fall partly inside and partly outside a 70 x 41 frame; 3 x 6 tiles."""
    width, height = 70, 41
    guide = ref.compose_guide(basic(width=width, height=height), width, height)
    rgb = oracle.render(basic(16, width=width, height=height), width, height, seed=SEED)[1]
    assert_filter_is_the_restatement(tracer, rgb, guide, ref.params(iterations=5, normal_squarings=5, sigma_colour=0.6, sigma_albedo=0.1, sigma_depth=0.05), "70x41")


def test_zero_iterations_pass_the_image_through_and_pack_it_as_rt_hip_render_does(tracer):
    rgba, rgb, _ = tracer.render(basic(16), W, H, seed=SEED, want_rgb=True)
    assert np.array_equal(rgba, noisy_basic()[1]) and np.array_equal(bits(rgb), bits(noisy_basic()[0]))
    got_rgb, got_rgba = device_filter(tracer, rgb, composed("basic_pinhole"), ref.params(iterations=0))
    assert np.array_equal(bits(got_rgb), bits(rgb))
    assert np.array_equal(got_rgba, rgba)
    # either output alone
    only_rgba = device_filter(tracer, rgb, composed("basic_pinhole"), ref.params(iterations=0), want_rgb=False)[1]
    assert np.array_equal(only_rgba, rgba)
    p = ref.params(iterations=3)
    want_rgb, want_rgba = ref.filter(rgb, composed("basic_pinhole"), p)
    assert np.array_equal(device_filter(tracer, rgb, composed("basic_pinhole"), p, want_rgb=False)[1], want_rgba)
    assert np.array_equal(bits(device_filter(tracer, rgb, composed("basic_pinhole"), p, want_rgba=False)[0]), bits(want_rgb))


def test_the_filters_refusals(tracer):
    import torch

    image = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda:0")
    guide = torch.zeros((H, W, 8), dtype=torch.float32, device="cuda:0")
    with pytest.raises(rt_amd.RtHipError) as refused:
        tracer.denoise_device(W, H, image.data_ptr(), guide.data_ptr(), None, None, None)
    assert refused.value.status == INVALID_ARGUMENT and "NULL" in str(refused.value)
    for out in (image.data_ptr(), image.data_ptr() + 12 * W):  # the very image, and one that starts a row further on
        with pytest.raises(rt_amd.RtHipError) as refused:
            tracer.denoise_device(W, H, image.data_ptr(), guide.data_ptr(), None, out, None)
        assert refused.value.status == INVALID_ARGUMENT and "overlap" in str(refused.value)
    with pytest.raises(rt_amd.RtHipError) as refused:
        tracer.denoise_device(W, H, image.data_ptr(), guide.data_ptr(), ref.params(iterations=7), None, image.data_ptr())
    assert refused.value.status == INVALID_ARGUMENT and "iterations" in str(refused.value)


# ---- the drop-in ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def one_shot(spp, tilted=False):
    rgba, rgb, _ = oracle.render(basic(spp, tilted), W, H, seed=SEED)
    return rgba, rgb


def test_denoise_progressive_follows_a_48_spp_frame_in_passes_of_16_and_leaves_it_alone():
    p = ref.params(iterations=3, normal_squarings=5, sigma_colour=0.6, sigma_albedo=0.1, sigma_depth=0.05)
    with rt_amd.HipRayTracer(device=0) as tracer:
        with pytest.raises(rt_amd.RtHipError) as refused:  # before any pass
            tracer.denoise_progressive(size=(W, H))
        assert refused.value.status == INVALID_ARGUMENT and "no accumulation in flight" in str(refused.value)
        for done in (16, 32, 48):
            rgba, rgb, _, progress = tracer.render_progressive(basic(48), W, H, seed=SEED, pass_samples=16, want_rgb=True)
            assert progress["samples_done"] == done
            # every pass's own frame is still the oracle's: the calls in between left the accumulation alone
            assert np.array_equal(rgba, one_shot(done)[0]) and np.array_equal(bits(rgb), bits(one_shot(done)[1]))
            for params in (p, None):  # (the second call finds the guide kept)
                got_rgba, got_rgb, ms = tracer.denoise_progressive(params, want_rgb=True)
                want_rgb, want_rgba = ref.filter(rgb, composed("basic_pinhole"), params)
                assert np.array_equal(bits(got_rgb), bits(want_rgb)), f"after {done} samples"
                assert np.array_equal(got_rgba, want_rgba)
                assert ms > 0.0
            assert np.array_equal(tracer.denoise_progressive(p)[0], ref.filter(rgb, composed("basic_pinhole"), p)[1])  # packed pixels alone
        # the accumulation is finished: the call still works, and a call on the finished frame still delivers it
        rgba, rgb, _, progress = tracer.render_progressive(basic(48), W, H, seed=SEED, pass_samples=16, want_rgb=True)
        assert progress["passes"] == 3 and np.array_equal(rgba, one_shot(48)[0]) and np.array_equal(bits(rgb), bits(one_shot(48)[1]))
        # a changed camera starts a new accumulation: a fresh guide
        rgba, rgb, _, progress = tracer.render_progressive(basic(48, tilted=True), W, H, seed=SEED, pass_samples=16, want_rgb=True)
        assert progress["restarted"] == 1 and np.array_equal(bits(rgb), bits(one_shot(16, True)[1]))
        got_rgba, got_rgb, _ = tracer.denoise_progressive(p, want_rgb=True)
        want_rgb, want_rgba = ref.filter(rgb, composed("basic_tilted_eye"), p)
        assert np.array_equal(bits(got_rgb), bits(want_rgb)) and np.array_equal(got_rgba, want_rgba)
        assert not np.array_equal(bits(composed("basic_tilted_eye")), bits(composed("basic_pinhole")))
        # ... and the pass after it continues as if nothing had happened
        rgba, rgb, _, progress = tracer.render_progressive(basic(48, tilted=True), W, H, seed=SEED, pass_samples=16, want_rgb=True)
        assert progress["samples_done"] == 32 and np.array_equal(bits(rgb), bits(one_shot(32, True)[1]))
    assert rt_amd.live_frame_locks() == 0


def test_denoise_progressive_on_a_multi_context_is_unsupported():
    with rt_amd.HipRayTracer(devices=[0], peer_copy=True) as multi:
        with pytest.raises(rt_amd.RtHipError) as refused:
            multi.denoise_progressive(size=(W, H))
        assert refused.value.status == UNSUPPORTED and "rt_hip_create" in str(refused.value)
    assert rt_amd.live_frame_locks() == 0


def test_the_plug_in_delivers_denoised_passes_and_rt_headless_writes_the_denoised_last_pass(tmp_path):
    """rt_headless --progressive 16 --denoise (RT_HIP_DENOISE=always): the file is the last pass through the default filter.  With
    RT_HIP_DENOISE=1 alone the finished frame is delivered as the path tracer made it."""
    binary = ROOT / "rt_amd" / "bin" / "rt_headless"
    common = [str(binary), "--renderer", "hip", "--scene", "basic.toml", "--size", f"{W}x{H}", "--spp", "48", "--progressive", "16"]
    env = dict(os.environ, RT_HIP_SEED=str(SEED))
    for name in ("RT_HIP_PROGRESSIVE", "RT_HIP_DENOISE"):
        env.pop(name, None)
    header = f"P6\n{W} {H}\n255\n".encode()
    want_denoised = unpack(ref.filter(one_shot(48)[1], composed("basic_pinhole"), None)[1])[..., :3]
    want_plain = unpack(one_shot(48)[0])[..., :3]
    assert not np.array_equal(want_denoised, want_plain)
    for extra, extra_env, want in ((["--denoise"], {}, want_denoised), ([], {"RT_HIP_DENOISE": "1"}, want_plain)):
        out = tmp_path / f"frame{len(extra)}.ppm"
        done = subprocess.run([*common, *extra, "--out", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=300, env=dict(env, **extra_env))
        assert done.returncode == 0 and "error" not in done.stderr, done.stderr
        data = out.read_bytes()
        assert data.startswith(header)
        assert np.array_equal(np.frombuffer(data[len(header) :], dtype=np.uint8).reshape(H, W, 3), want)
