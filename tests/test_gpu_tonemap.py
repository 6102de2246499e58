"""Tone mapping on the GPU, tolerance 0 throughout: the three launches (rt_hip_tonemap_device) against the serial CPU
restatement over the kernels' own text (tests/tonemap_reference.py) — the bit patterns of the float frame, the packed pixels and all
eight words of the state record — and the drop-in (rt_hip_render_tonemapped) against rt_hip_render's own float frame pushed through
the restatement."""
import functools

import numpy as np
import pytest

import rt_amd
from rt_amd import capi
from tests import light_reference as light_ref
from tests import tonemap_reference as ref

pytestmark = pytest.mark.gpu

F32 = np.float32
INVALID_ARGUMENT, UNSUPPORTED = 1, 5
EMISSION, DIRECT, SM = capi.RT_HIP_FLAG_EMISSION, capi.RT_HIP_FLAG_DIRECT_LIGHT, capi.RT_HIP_FLAG_SM_MATERIALS
BLOCK, GRID_PER_COMPUTE_UNIT = 256, 2  # luminance_histogram: 256 lanes a workgroup, 4 pixels a lane and trip, at most 2 workgroups per compute unit


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def device_tonemap(tracer, rgb, p, state=None, in_place=False, want_rgb=True, want_rgba=True):
    """rt_hip_tonemap_device on copies of the arrays -> (mapped float32 or None, rgba uint32 or None, state uint32[8])."""
    import torch

    device = f"cuda:{tracer.device}"
    height, width = rgb.shape[:2]
    d_in = torch.from_numpy(np.array(rgb, dtype=F32)).to(device)
    d_state = torch.from_numpy((np.zeros(8, dtype=np.uint32) if state is None else np.array(state, dtype=np.uint32)).view(np.int32)).to(device)
    d_out = d_in if in_place else (torch.full((height, width, 3), float("nan"), dtype=torch.float32, device=device) if want_rgb else None)
    d_rgba = torch.zeros((height, width), dtype=torch.int32, device=device) if want_rgba else None
    tracer.tonemap_device(width, height, d_in.data_ptr(), d_state.data_ptr(), p, d_out.data_ptr() if d_out is not None else None, d_rgba.data_ptr() if want_rgba else None, stream=stream())
    if not in_place:
        assert np.array_equal(bits(d_in.cpu().numpy()), bits(rgb))  # (the input is not touched)
    return (d_out.cpu().numpy() if d_out is not None else None), (d_rgba.cpu().numpy().view(np.uint32) if want_rgba else None), d_state.cpu().numpy().view(np.uint32)


def assert_is_the_restatement(tracer, rgb, p, what, state=None, **how):
    got_rgb, got_rgba, got_state = device_tonemap(tracer, rgb, p, state, **how)
    want_rgb, want_rgba, want_state = ref.frame(rgb, p, state)
    assert np.array_equal(got_state, want_state), f"{what}: state {ref.info_of(got_state)} {got_state[6:]}, the restatement's {ref.info_of(want_state)}"
    if got_rgb is not None:
        differing = (bits(got_rgb) != bits(want_rgb)).any(axis=-1)
        assert not differing.any(), f"{what}: {differing.sum()} of {differing.size} pixels differ from the restatement, first at (y, x) = {tuple(np.argwhere(differing)[0])}"
    if got_rgba is not None:
        assert np.array_equal(got_rgba, want_rgba), what
    return got_rgb, got_rgba, got_state


# ---- the device entry -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lights", "lights_sm", "basic"])
def test_the_fixture_frames(tracer, name):
    for curve in ref.CURVES:
        assert_is_the_restatement(tracer, ref.fixture_frames()[name], ref.params(curve=curve), f"{name} / curve {curve}")


# one pixel; a tail and no whole run of 4; three runs and a tail of 3; one workgroup's lanes plus a pixel
@pytest.mark.parametrize("width,height", [(1, 1), (1, 7), (7, 1), (5, 3), (257, 1), (1025, 1)])
def test_ragged_noise_frames(tracer, width, height):
    rgb = ref.noise(height, width, seed=100 * width + height)
    for curve in ref.CURVES:
        assert_is_the_restatement(tracer, rgb, ref.params(curve=curve), f"{width}x{height} / curve {curve}")
    assert_is_the_restatement(tracer, rgb, ref.params(low_permille=0, high_permille=0), f"{width}x{height} untrimmed")


def test_a_frame_past_one_trip_of_the_capped_grid(tracer):
    """1024 x 520: 133120 runs of 4 pixels.  The grid is min(ceil(runs / 256), 2 x compute units) workgroups of 256 lanes: on every device
    with at most 259 compute units some lanes take a second run — which this asserts is so here, from that rule and the device."""
    import torch

    width, height = 1024, 520
    compute_units = torch.cuda.get_device_properties(tracer.device).multi_processor_count
    runs = width * height // 4
    grid = min(-(-runs // BLOCK), GRID_PER_COMPUTE_UNIT * compute_units)
    assert grid * BLOCK < runs, f"{compute_units} compute units: one trip of {grid} workgroups covers the frame's {runs} runs"
    rgb = ref.noise(height, width, seed=9)
    _, _, state = assert_is_the_restatement(tracer, rgb, ref.params(), "1024x520")
    assert ref.info_of(state)["counted"] == width * height


@functools.lru_cache(maxsize=None)
def cases():
    return ref.constructed_cases()


@pytest.mark.parametrize("name", list(ref.constructed_cases()))
def test_the_constructed_cases(tracer, name):
    rgb, p = cases()[name]
    _, _, state = assert_is_the_restatement(tracer, rgb, p, name)
    if name == "all skipped":
        assert ref.info_of(state) == {"exposure": 1.0, "target": 1.0, "counted": 0, "skipped": 35, "kept": 0, "mean_q8": 0}
    if name == "manual exposure":
        assert not state[2:].any()


def test_a_wave_in_one_bin_and_a_wave_alternating_between_two(tracer):
    """A lane takes 4 consecutive pixels, a wave 256: a flat frame puts all 64 lanes of every wave on ONE LDS word; runs of 4 pixels
    that alternate between two values put the even lanes on one word and the odd lanes on another."""
    flat = ref.grey(4, 256, [ref.bin_centre(131)])
    _, _, state = assert_is_the_restatement(tracer, flat, ref.params(low_permille=0, high_permille=0), "flat")
    assert ref.info_of(state)["mean_q8"] == 131 * 256 and ref.info_of(state)["counted"] == 1024
    lane = (np.arange(1024) // 4) % 64
    values = np.where(lane % 2 == 0, F32(ref.bin_centre(90)), F32(ref.bin_centre(170)))
    alternating = np.repeat(values.reshape(4, 256, 1), 3, axis=2).astype(F32)
    _, _, state = assert_is_the_restatement(tracer, alternating, ref.params(low_permille=0, high_permille=0), "alternating")
    assert ref.info_of(state)["mean_q8"] == 130 * 256
    assert np.array_equal(ref.histogram(alternating)[[90, 170]], [512, 512])


def test_in_place_and_either_output_alone(tracer):
    rgb = ref.fixture_frames()["lights"]
    for curve in ref.CURVES:
        p = ref.params(curve=curve)
        assert_is_the_restatement(tracer, rgb, p, "in place", in_place=True)
        assert_is_the_restatement(tracer, rgb, p, "float only", want_rgba=False)
        assert_is_the_restatement(tracer, rgb, p, "packed only", want_rgb=False)


def test_what_the_device_entry_refuses(tracer):
    import torch

    device = f"cuda:{tracer.device}"
    d = torch.zeros(64 * 36 * 3 + 64, dtype=torch.float32, device=device)
    d_state = torch.zeros(8, dtype=torch.int32, device=device)
    d_rgba = torch.zeros(64 * 36, dtype=torch.int32, device=device)
    base, s = d.data_ptr(), stream()
    assert base % 16 == 0
    refusals = [
        (dict(d_rgb_in=base, d_rgb_out=base + 16, d_rgba8_out=None), "d_rgb_out overlaps d_rgb_in"),  # partial overlap: 4 floats on
        (dict(d_rgb_in=base + 16, d_rgb_out=base, d_rgba8_out=None), "d_rgb_out overlaps d_rgb_in"),
        (dict(d_rgb_in=base, d_rgb_out=None, d_rgba8_out=base + 64), "d_rgba8_out overlaps d_rgb_in"),
        (dict(d_rgb_in=base, d_rgb_out=base, d_rgba8_out=base), "d_rgba8_out overlaps d_rgb_in"),
        (dict(d_rgb_in=base + 4, d_rgb_out=None, d_rgba8_out=d_rgba.data_ptr()), "d_rgb_in is not 16-byte aligned"),
        (dict(d_rgb_in=base + 12, d_rgb_out=base + 12, d_rgba8_out=None), "d_rgb_in is not 16-byte aligned"),
        (dict(d_rgb_in=base, d_rgb_out=None, d_rgba8_out=None), "both NULL"),
        (dict(d_rgb_in=None, d_rgb_out=base, d_rgba8_out=None), "NULL argument"),
    ]
    for arguments, words in refusals:
        with pytest.raises(capi.RtHipError) as refused:
            tracer.tonemap_device(64, 36, arguments["d_rgb_in"], d_state.data_ptr(), None, arguments["d_rgb_out"], arguments["d_rgba8_out"], stream=s)
        assert refused.value.status == INVALID_ARGUMENT and words in str(refused.value) and "rt_hip_tonemap_device" in str(refused.value), (words, str(refused.value))
    with pytest.raises(capi.RtHipError) as refused:  # the state record inside the input
        tracer.tonemap_device(64, 36, base, base + 32, None, None, d_rgba.data_ptr(), stream=s)
    assert refused.value.status == INVALID_ARGUMENT and "d_state overlaps d_rgb_in" in str(refused.value)
    with pytest.raises(capi.RtHipError) as refused:
        tracer.tonemap_device(0, 36, base, d_state.data_ptr(), None, None, d_rgba.data_ptr(), stream=s)
    assert refused.value.status == INVALID_ARGUMENT and "frame 0x36" in str(refused.value)
    torch.cuda.synchronize()
    assert not d.cpu().numpy().any() and not d_rgba.cpu().numpy().any() and not d_state.cpu().numpy().any()  # nothing was launched


def test_the_bins_are_cleared_and_a_frame_twice_is_the_same_bytes(tracer):
    """The histogram scratch is the context's and dirty from whatever ran before: a frame after another frame, and the same frame again,
    give the restatement's bytes each time."""
    dirty, rgb = ref.noise(70, 41, seed=21), ref.fixture_frames()["lights"]
    p = ref.params(curve=ref.REINHARD)
    assert_is_the_restatement(tracer, dirty, p, "the frame before")
    first = assert_is_the_restatement(tracer, rgb, p, "on a dirty scratch")
    second = assert_is_the_restatement(tracer, rgb, p, "again")
    for a, b in zip(first, second):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_three_calls_adapt_on_one_state_record(tracer):
    import torch

    device = f"cuda:{tracer.device}"
    p = ref.params(adaptation=0.25)
    frames = [ref.fixture_frames()[name] for name in ("lights", "basic", "lights_sm")]
    d_state = torch.zeros(8, dtype=torch.int32, device=device)  # zeroed: the first call starts at its target
    want_state = np.zeros(8, dtype=np.uint32)
    exposures = []
    for number, rgb in enumerate(frames):
        d_in = torch.from_numpy(np.array(rgb, dtype=F32)).to(device)
        d_rgba = torch.zeros(rgb.shape[:2], dtype=torch.int32, device=device)
        tracer.tonemap_device(64, 36, d_in.data_ptr(), d_state.data_ptr(), p, d_in.data_ptr(), d_rgba.data_ptr(), stream=stream())
        want_rgb, want_rgba, want_state = ref.frame(rgb, p, want_state)
        assert np.array_equal(d_state.cpu().numpy().view(np.uint32), want_state), number
        assert np.array_equal(bits(d_in.cpu().numpy()), bits(want_rgb)) and np.array_equal(d_rgba.cpu().numpy().view(np.uint32), want_rgba), number
        exposures.append(ref.info_of(want_state)["exposure"])
    assert exposures[0] == ref.info_of(ref.frame(frames[0], p)[2])["target"] and len(set(exposures)) == 3
    assert exposures[1] != ref.info_of(ref.frame(frames[1], p)[2])["exposure"]  # (the second call did ease from the first)


def test_on_a_multi_context_the_root_member_answers(tracer):
    with rt_amd.HipRayTracer(devices=[0], peer_copy=True) as multi:
        assert_is_the_restatement(multi, ref.fixture_frames()["lights"], None, "multi")


# ---- the drop-in --------------------------------------------------------------------------------------------------------------------
def lights_pod():
    return light_ref.lights_scene(spp=20).describe(64, 36)


def basic_pod():
    return rt_amd.Scene.named("basic").set_sampling(4).describe(64, 36)


DROP_IN = {"emission": (lights_pod, EMISSION), "direct light": (lights_pod, EMISSION | DIRECT), "sm materials": (lights_pod, EMISSION | SM), "basic": (basic_pod, 0)}
_traced = {}


@pytest.fixture
def lit(tracer):
    tracer.set_emission(light_ref.LIGHTS_TABLE)
    yield tracer
    tracer.set_emission(None)  # (the session's context is shared: no other test file sees a table)


def traced(tracer, case, seed=11):
    """rt_hip_render's frame of a case — packed pixels and float mean — computed once, shared, read-only."""
    if case not in _traced:
        make, flags = DROP_IN[case]
        rgba, rgb, _ = tracer.render(make(), 64, 36, seed=seed, flags=flags, want_rgb=True)
        rgba.setflags(write=False), rgb.setflags(write=False)
        _traced[case] = (rgba, rgb)
    return _traced[case]


@pytest.mark.parametrize("case", list(DROP_IN))
def test_the_drop_in_is_rt_hip_render_through_the_restatement(lit, case):
    make, flags = DROP_IN[case]
    _, mean = traced(lit, case)
    for curve in ref.CURVES:
        p = ref.params(curve=curve)
        rgba, rgb, stats, info = lit.render_tonemapped(make(), 64, 36, seed=11, flags=flags, params=p, want_rgb=True)
        want_rgb, want_rgba, want_state = ref.frame(mean, p)
        assert info == ref.info_of(want_state), (case, curve)
        assert np.array_equal(bits(rgb), bits(want_rgb)) and np.array_equal(rgba, want_rgba), (case, curve)
        assert stats["primary_samples"] == 64 * 36 * make().samples_per_pixel and stats["render_ms"] > 0.0
        only_pixels, no_rgb, _, same_info = lit.render_tonemapped(make(), 64, 36, seed=11, flags=flags, params=p, stats=False)
        assert no_rgb is None and np.array_equal(only_pixels, want_rgba) and same_info == info
    manual = ref.params(curve=ref.REINHARD, exposure=0.5)
    rgba, rgb, _, info = lit.render_tonemapped(make(), 64, 36, seed=11, flags=flags, params=manual, want_rgb=True)
    want_rgb, want_rgba, want_state = ref.frame(mean, manual)
    assert info == ref.info_of(want_state) == {"exposure": 0.5, "target": 0.5, "counted": 0, "skipped": 0, "kept": 0, "mean_q8": 0}
    assert np.array_equal(bits(rgb), bits(want_rgb)) and np.array_equal(rgba, want_rgba)


def test_the_lit_frame_is_no_longer_flat_white(lit):
    plain, mean = traced(lit, "emission")
    mapped, _, _, _ = lit.render_tonemapped(lights_pod(), 64, 36, seed=11, flags=EMISSION, params=ref.params(curve=ref.ACES))
    assert not np.array_equal(mapped, plain)
    from tests.conftest import unpack

    assert (unpack(mapped)[..., :3] == 255).sum() < (unpack(plain)[..., :3] == 255).sum()
    assert (mean > 1).mean() > 0.05  # (there was something to map)


def test_a_size_change_resets_the_kept_exposure():
    eased = ref.params(adaptation=0.25)
    with rt_amd.HipRayTracer(device=0) as t:
        t.set_emission(light_ref.LIGHTS_TABLE)
        lights_64 = t.render(lights_pod(), 64, 36, seed=11, flags=EMISSION, want_rgb=True)[1]
        basic_64 = t.render(basic_pod(), 64, 36, seed=11, want_rgb=True)[1]
        small = rt_amd.Scene.named("basic").set_sampling(4).describe(32, 18)
        basic_32 = t.render(small, 32, 18, seed=11, want_rgb=True)[1]
        state = np.zeros(8, dtype=np.uint32)
        _, _, _, first = t.render_tonemapped(lights_pod(), 64, 36, seed=11, flags=EMISSION, params=eased)
        state = ref.frame(lights_64, eased, state)[2]
        assert first == ref.info_of(state) and first["exposure"] == first["target"]
        _, _, _, second = t.render_tonemapped(basic_pod(), 64, 36, seed=11, params=eased)
        state = ref.frame(basic_64, eased, state)[2]
        assert second == ref.info_of(state) and second["exposure"] != second["target"]  # eased from the lights frame's
        _, _, _, third = t.render_tonemapped(small, 32, 18, seed=11, params=eased)  # another size: the record starts over
        assert third == ref.info_of(ref.frame(basic_32, eased)[2]) and third["exposure"] == third["target"]
        _, _, _, fourth = t.render_tonemapped(basic_pod(), 64, 36, seed=11, params=eased)  # ... and again on the way back
        assert fourth == ref.info_of(ref.frame(basic_64, eased)[2]) and fourth["exposure"] == fourth["target"]


def test_what_the_drop_in_refuses(tracer):
    pod = basic_pod()
    for flag, named in ((capi.RT_HIP_FLAG_PREVIEW, "RT_HIP_FLAG_PREVIEW"), (capi.RT_HIP_FLAG_PERSISTENT_FRAME, "RT_HIP_FLAG_PERSISTENT_FRAME"), (1 << 30, "unknown flag bits")):
        with pytest.raises(capi.RtHipError) as refused:
            tracer.render_tonemapped(pod, 64, 36, seed=1, flags=flag)
        assert refused.value.status == UNSUPPORTED and named in str(refused.value) and "rt_hip_render_tonemapped" in str(refused.value)
    with pytest.raises(capi.RtHipError) as refused:
        tracer.render_tonemapped(pod, 0, 36, seed=1)
    assert refused.value.status == INVALID_ARGUMENT and "frame 0x36" in str(refused.value)
    with pytest.raises(capi.RtHipError) as refused:  # lights without a table: the launch's own refusal comes through
        tracer.render_tonemapped(pod, 64, 36, seed=1, flags=EMISSION)
    assert refused.value.status == INVALID_ARGUMENT and "RT_HIP_FLAG_EMISSION without an emission table" in str(refused.value)
    with rt_amd.HipRayTracer(devices=[0], peer_copy=True) as multi:
        with pytest.raises(capi.RtHipError) as refused:
            multi.render_tonemapped(pod, 64, 36, seed=1)
        assert refused.value.status == UNSUPPORTED and "rt_hip_create" in str(refused.value) and "rt_hip_render_tonemapped" in str(refused.value)
    assert rt_amd.live_frame_locks() == 0


# ---- interleaved with the other drop-in calls (in the manner of test_gpu_drop_in_interleave.py) -----------------------------------------
def interleave_calls(t):
    p = rt_amd.Scene.named("basic").set_sampling(32).describe(64, 36)
    eased = ref.params(adaptation=0.5)
    return {
        "render": lambda: t.render(p, 64, 36, seed=7, want_rgb=True),
        "tonemapped 1": lambda: t.render_tonemapped(p, 64, 36, seed=7, params=eased, want_rgb=True),
        "tonemapped 2": lambda: t.render_tonemapped(p, 64, 36, seed=8, params=eased, want_rgb=True),
        "upscaled": lambda: t.render_upscaled(p, 64, 36, seed=7, factor=2, want_rgb=True),
        "render again": lambda: t.render(p, 64, 36, seed=9, want_rgb=True),
    }


def test_interleaved_with_render_and_render_upscaled_each_frame_is_what_it_is_alone():
    interleaved = ["tonemapped 1", "render", "upscaled", "tonemapped 2", "render again"]
    alone = ["render", "render again", "upscaled", "tonemapped 1", "tonemapped 2"]

    def run(order):
        with rt_amd.HipRayTracer(device=0) as t:
            todo = interleave_calls(t)
            return {label: todo[label]() for label in order}

    a, b = run(interleaved), run(alone)
    for label in interleaved:
        for x, y in zip(a[label], b[label]):
            if isinstance(x, np.ndarray):
                assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), label
            elif "render_ms" in x:
                assert {k: x[k] for k in ("segments", "primary_samples", "kernel_variant")} == {k: y[k] for k in ("segments", "primary_samples", "kernel_variant")}, label
            else:
                assert x == y, label
    # the kept exposure went from the first tone-mapped frame to the second across the calls in between
    assert a["tonemapped 2"][3]["exposure"] != a["tonemapped 2"][3]["target"]
    want = ref.frame(a["render"][1], ref.params(adaptation=0.5))
    assert np.array_equal(a["tonemapped 1"][0], want[1]) and np.array_equal(bits(a["tonemapped 1"][1]), bits(want[0]))
    assert rt_amd.live_frame_locks() == 0
