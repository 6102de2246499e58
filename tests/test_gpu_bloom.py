"""Bloom on the GPU, tolerance 0 throughout: the 2 x levels launches (rt_hip_bloom_device) against the serial CPU
restatement over the kernels' own text (tests/bloom_reference.py) — the bit patterns of the frame and of the glow layer — and the
drop-in (rt_hip_render_bloomed) against rt_hip_render's own float frame pushed through the bloom restatement and then the tone-mapping
restatement."""
import functools

import numpy as np
import pytest

import rt_amd
from rt_amd import capi
from tests import bloom_reference as ref
from tests import light_reference as light_ref
from tests import tonemap_reference as tonemap_ref

pytestmark = pytest.mark.gpu

F32 = np.float32
INVALID_ARGUMENT, UNSUPPORTED = 1, 5
EMISSION, DIRECT, SM = capi.RT_HIP_FLAG_EMISSION, capi.RT_HIP_FLAG_DIRECT_LIGHT, capi.RT_HIP_FLAG_SM_MATERIALS
SENTINEL = 0x7FC0BEEF  # a NaN with a payload: an untouched float keeps these bits


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def device_bloom(tracer, rgb, p, in_place=False, want_rgb=True, want_layer=True):
    """rt_hip_bloom_device on copies of the arrays -> (frame float32 or None, layer float32 or None).  Both outputs lie in the middle of
    sentinel-filled blocks: nothing outside them may be written, and the input is untouched when the call is not in place."""
    import torch

    device = f"cuda:{tracer.device}"
    height, width = rgb.shape[:2]
    n, pad = height * width * 3, 64
    d_in = torch.from_numpy(np.array(rgb, dtype=F32)).to(device)

    def block():
        return torch.full((n + 2 * pad,), SENTINEL, dtype=torch.int32, device=device)

    d_out = None if in_place or not want_rgb else block()
    d_layer = block() if want_layer else None
    out_ptr = d_in.data_ptr() if in_place else (d_out.data_ptr() + 4 * pad if d_out is not None else None)
    tracer.bloom_device(width, height, d_in.data_ptr(), p, out_ptr, d_layer.data_ptr() + 4 * pad if want_layer else None, stream=stream())

    def middle(d):
        words = d.cpu().numpy().view(np.uint32)
        assert (words[:pad] == SENTINEL).all() and (words[-pad:] == SENTINEL).all(), "something outside an output was written"
        return words[pad:-pad].view(F32).reshape(height, width, 3)

    if not in_place:
        assert np.array_equal(bits(d_in.cpu().numpy()), bits(rgb))  # (the input is not touched)
    got = d_in.cpu().numpy() if in_place else (middle(d_out) if d_out is not None else None)
    return got, (middle(d_layer) if want_layer else None)


@functools.lru_cache(maxsize=None)
def restated(key):
    """The restatement of a registered frame, computed once and shared (read-only)."""
    rgb, p = _registered[key]
    out, layer = ref.frame(rgb, p)
    out.setflags(write=False), layer.setflags(write=False)
    return out, layer


_registered = {}


def assert_is_the_restatement(tracer, rgb, p, what, **how):
    _registered[what] = (rgb, p)
    want_out, want_layer = restated(what)
    got_out, got_layer = device_bloom(tracer, rgb, p, **how)
    for name, got, want in (("frame", got_out, want_out), ("layer", got_layer, want_layer)):
        if got is not None:
            differing = (bits(got) != bits(want)).any(axis=-1)
            assert not differing.any(), f"{what}: {differing.sum()} of {differing.size} {name} pixels differ from the restatement, first at (y, x) = {tuple(np.argwhere(differing)[0])}"
    return got_out, got_layer


# ---- the device entry -------------------------------------------------------------------------------------------------------------
# one texel; levels of one row or one column; 16 x 16: exactly one bloom_down tile from level 0 on; 67 x 35: level 1 is 17 wide, one texel
# past a tile; 65 x 65: level 1 is 17 x 17, a tile corner and four workgroups; 130 x 66: level 1 is 33 wide, three tile columns; 257 x 255:
# several 64 x 4 strips both ways, ragged; 1 x 32768 and 32768 x 1: every level ragged, thousands of strips or tiles along one axis
@pytest.mark.parametrize("width,height", [(1, 1), (1, 2), (2, 1), (3, 3), (16, 16), (67, 35), (65, 65), (130, 66), (257, 255), (1, 32768), (32768, 1)])
def test_noise_frames(tracer, width, height):
    rgb = ref.noise(height, width, seed=100 * (width % 1000) + height % 1000)
    assert_is_the_restatement(tracer, rgb, ref.params(levels=8), f"noise {width}x{height}")


@pytest.mark.parametrize("name", list(ref.constructed_cases()))
def test_the_constructed_cases(tracer, name):
    rgb, p = ref.constructed_cases()[name]
    out, layer = assert_is_the_restatement(tracer, rgb, p, name)
    if name == "hostile pixels":
        assert np.isnan(out).sum() == 1 and np.isfinite(layer).all()
        clean_layer = restated_of(tracer, "hostile pixels, as the bright pass takes them")[1]
        assert np.array_equal(bits(layer), bits(clean_layer))
    if name == "denormals":
        assert (layer > 0).all()  # (nothing was flushed to zero on the way)


def restated_of(tracer, name):
    rgb, p = ref.constructed_cases()[name]
    _registered[name] = (rgb, p)
    return restated(name)


def test_in_place_layer_only_frame_only(tracer):
    rgb = ref.noise(35, 67, seed=41)
    p = ref.params()
    assert_is_the_restatement(tracer, rgb, p, "67x35 defaults", in_place=True)
    assert_is_the_restatement(tracer, rgb, p, "67x35 defaults", in_place=True, want_layer=False)
    assert_is_the_restatement(tracer, rgb, p, "67x35 defaults", want_rgb=False)
    assert_is_the_restatement(tracer, rgb, p, "67x35 defaults", want_layer=False)
    assert_is_the_restatement(tracer, rgb, None, "67x35 defaults")  # (NULL: the defaults)


def test_one_level_and_a_clipped_eight(tracer):
    rgb = ref.noise(35, 67, seed=42)
    assert ref.plan(67, 35, ref.params(levels=1))["levels"] == 1 and ref.plan(67, 35, ref.params(levels=8))["levels"] == 7
    assert_is_the_restatement(tracer, rgb, ref.params(levels=1), "67x35 one level")
    assert_is_the_restatement(tracer, rgb, ref.params(levels=8), "67x35 eight asked for")
    assert_is_the_restatement(tracer, rgb, ref.params(levels=8, scatter=1.0, knee=0.0, threshold=0.25, intensity=3.0), "67x35 wide")
    assert_is_the_restatement(tracer, rgb, ref.params(scatter=0.0), "67x35 tight")


def test_two_sizes_on_one_context_share_the_scratch():
    """A context of its own: the small frame reserves a small pyramid, the large one re-reserves it, the small one then runs in the large
    block over whatever the large frame left there — each time the restatement's bytes."""
    small, large = ref.noise(9, 13, seed=43), ref.noise(130, 200, seed=44)
    with rt_amd.HipRayTracer(device=0) as t:
        for what, rgb in (("13x9", small), ("200x130", large), ("13x9", small), ("200x130", large)):
            assert_is_the_restatement(t, rgb, ref.params(levels=8), what)


def test_on_a_multi_context_the_root_member_answers():
    with rt_amd.HipRayTracer(devices=[0], peer_copy=True) as multi:
        assert_is_the_restatement(multi, ref.noise(21, 37, seed=45), None, "multi 37x21")


def test_what_the_device_entry_refuses(tracer):
    import torch

    device = f"cuda:{tracer.device}"
    d = torch.zeros(2 * 64 * 36 * 3 + 64, dtype=torch.float32, device=device)
    base, s, frame_bytes = d.data_ptr(), stream(), 64 * 36 * 12
    other = base + frame_bytes + 64
    refusals = [
        (dict(d_rgb_in=base, d_rgb_out=base + 16, d_layer_out=None), "d_rgb_out overlaps d_rgb_in"),
        (dict(d_rgb_in=base + 16, d_rgb_out=base, d_layer_out=None), "d_rgb_out overlaps d_rgb_in"),
        (dict(d_rgb_in=base, d_rgb_out=None, d_layer_out=base + 64), "d_layer_out overlaps d_rgb_in"),
        (dict(d_rgb_in=base, d_rgb_out=base, d_layer_out=base), "d_layer_out overlaps d_rgb_in"),
        (dict(d_rgb_in=base, d_rgb_out=other, d_layer_out=other + 12), "d_rgb_out"),  # two outputs on one another
        (dict(d_rgb_in=base + 2, d_rgb_out=None, d_layer_out=other), "not 4-byte aligned"),
        (dict(d_rgb_in=base, d_rgb_out=None, d_layer_out=None), "both NULL"),
        (dict(d_rgb_in=None, d_rgb_out=other, d_layer_out=None), "NULL argument"),
    ]
    for arguments, words in refusals:
        with pytest.raises(capi.RtHipError) as refused:
            tracer.bloom_device(64, 36, arguments["d_rgb_in"], None, arguments["d_rgb_out"], arguments["d_layer_out"], stream=s)
        assert refused.value.status == INVALID_ARGUMENT and words in str(refused.value) and "rt_hip_bloom_device" in str(refused.value), (words, str(refused.value))
    for width, height in ((0, 36), (64, 0), (32769, 1)):
        with pytest.raises(capi.RtHipError) as refused:
            tracer.bloom_device(width, height, base, None, other, None, stream=s)
        assert refused.value.status == INVALID_ARGUMENT and f"frame {width}x{height}" in str(refused.value)
    with pytest.raises(capi.RtHipError) as refused:
        tracer.bloom_device(64, 36, base, ref.params(knee=2.0), other, None, stream=s)
    assert refused.value.status == INVALID_ARGUMENT and "knee" in str(refused.value)
    torch.cuda.synchronize()
    assert not d.cpu().numpy().any()  # nothing was launched


# ---- the drop-in --------------------------------------------------------------------------------------------------------------------
def lights_pod():
    return light_ref.lights_scene(spp=20).describe(64, 36)


DROP_IN = {"emission": EMISSION, "direct light": EMISSION | DIRECT, "sm materials": EMISSION | SM, "direct light, sm": EMISSION | DIRECT | SM}
_traced = {}


@pytest.fixture
def lit(tracer):
    tracer.set_emission(light_ref.LIGHTS_TABLE)
    yield tracer
    tracer.set_emission(None)  # (the session's context is shared: no other test file sees a table)


def traced(tracer, case, seed=11):
    """rt_hip_render's float mean of a case, computed once, shared, read-only."""
    if case not in _traced:
        _, rgb, _ = tracer.render(lights_pod(), 64, 36, seed=seed, flags=DROP_IN[case], want_rgb=True)
        rgb.setflags(write=False)
        _traced[case] = rgb
    return _traced[case]


@pytest.mark.parametrize("case", list(DROP_IN))
def test_the_drop_in_is_rt_hip_render_through_both_restatements(lit, case):
    flags, mean = DROP_IN[case], traced(lit, case)
    assert (mean > 1).mean() > 0.05  # (there is something to bloom)
    for bloom, curve in ((ref.params(), tonemap_ref.ACES), (ref.params(intensity=0.5, scatter=1.0, levels=8), tonemap_ref.REINHARD), (ref.params(levels=1), tonemap_ref.NONE)):
        p = tonemap_ref.params(curve=curve)
        rgba, rgb, stats, info = lit.render_bloomed(lights_pod(), 64, 36, seed=11, flags=flags, bloom_params=bloom, tonemap_params=p, want_rgb=True)
        bloomed, _ = ref.frame(mean, bloom)
        want_rgb, want_rgba, want_state = tonemap_ref.frame(bloomed, p)
        assert info == tonemap_ref.info_of(want_state), (case, curve)
        assert np.array_equal(bits(rgb), bits(want_rgb)) and np.array_equal(rgba, want_rgba), (case, curve)
        assert stats["primary_samples"] == 64 * 36 * 20 and stats["render_ms"] > 0.0
        only_pixels, no_rgb, _, same_info = lit.render_bloomed(lights_pod(), 64, 36, seed=11, flags=flags, bloom_params=bloom, tonemap_params=p, stats=False)
        assert no_rgb is None and np.array_equal(only_pixels, want_rgba) and same_info == info
    assert not np.array_equal(bits(bloomed), bits(mean))  # (the glow is not nothing)


def test_with_intensity_0_it_is_rt_hip_render_tonemapped(lit):
    for case, flags in DROP_IN.items():
        p = tonemap_ref.params(curve=tonemap_ref.ACES)
        a = lit.render_bloomed(lights_pod(), 64, 36, seed=11, flags=flags, bloom_params=ref.params(intensity=0.0), tonemap_params=p, want_rgb=True)
        b = lit.render_tonemapped(lights_pod(), 64, 36, seed=11, flags=flags, params=p, want_rgb=True)
        assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])) and a[3] == b[3], case


def test_the_kept_exposure_eases_and_restarts_on_a_size_change():
    eased, bloom = tonemap_ref.params(adaptation=0.25), ref.params()
    basic = lambda w, h: rt_amd.Scene.named("basic").set_sampling(4).describe(w, h)
    with rt_amd.HipRayTracer(device=0) as t:
        t.set_emission(light_ref.LIGHTS_TABLE)
        lights_64 = ref.frame(t.render(lights_pod(), 64, 36, seed=11, flags=EMISSION, want_rgb=True)[1], bloom)[0]
        basic_64 = ref.frame(t.render(basic(64, 36), 64, 36, seed=11, want_rgb=True)[1], bloom)[0]
        basic_32 = ref.frame(t.render(basic(32, 18), 32, 18, seed=11, want_rgb=True)[1], bloom)[0]
        _, _, _, tonemapped = t.render_tonemapped(lights_pod(), 64, 36, seed=11, flags=EMISSION, params=eased)  # (its record is another one)
        _, _, _, first = t.render_bloomed(lights_pod(), 64, 36, seed=11, flags=EMISSION, bloom_params=bloom, tonemap_params=eased)
        state = tonemap_ref.frame(lights_64, eased)[2]
        assert first == tonemap_ref.info_of(state) and first["exposure"] == first["target"]
        _, _, _, second = t.render_bloomed(basic(64, 36), 64, 36, seed=11, bloom_params=bloom, tonemap_params=eased)
        state = tonemap_ref.frame(basic_64, eased, state)[2]
        assert second == tonemap_ref.info_of(state) and second["exposure"] != second["target"]  # eased from the lights frame's
        _, _, _, third = t.render_bloomed(basic(32, 18), 32, 18, seed=11, bloom_params=bloom, tonemap_params=eased)  # another size: the record starts over
        assert third == tonemap_ref.info_of(tonemap_ref.frame(basic_32, eased)[2]) and third["exposure"] == third["target"]
        # rt_hip_render_tonemapped's record did not see any of this: its second frame eases from ITS first
        _, _, _, again = t.render_tonemapped(lights_pod(), 64, 36, seed=11, flags=EMISSION, params=eased)
        assert again["exposure"] == tonemapped["exposure"] == tonemapped["target"]
    assert rt_amd.live_frame_locks() == 0


def test_what_the_drop_in_refuses(tracer):
    pod = rt_amd.Scene.named("basic").set_sampling(4).describe(64, 36)
    for flag, named in ((capi.RT_HIP_FLAG_PREVIEW, "RT_HIP_FLAG_PREVIEW"), (capi.RT_HIP_FLAG_PERSISTENT_FRAME, "RT_HIP_FLAG_PERSISTENT_FRAME"), (1 << 30, "unknown flag bits")):
        with pytest.raises(capi.RtHipError) as refused:
            tracer.render_bloomed(pod, 64, 36, seed=1, flags=flag)
        assert refused.value.status == UNSUPPORTED and named in str(refused.value) and "rt_hip_render_bloomed" in str(refused.value)
    with pytest.raises(capi.RtHipError) as refused:  # lights without a table: the launch's own refusal comes through
        tracer.render_bloomed(pod, 64, 36, seed=1, flags=EMISSION)
    assert refused.value.status == INVALID_ARGUMENT and "RT_HIP_FLAG_EMISSION without an emission table" in str(refused.value)
    with rt_amd.HipRayTracer(devices=[0], peer_copy=True) as multi:
        with pytest.raises(capi.RtHipError) as refused:
            multi.render_bloomed(pod, 64, 36, seed=1)
        assert refused.value.status == UNSUPPORTED and "rt_hip_create" in str(refused.value) and "rt_hip_render_bloomed" in str(refused.value)
    assert rt_amd.live_frame_locks() == 0
