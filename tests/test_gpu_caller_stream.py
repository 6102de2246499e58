"""Every device-level call on a CALLER'S stream behind pending work (include/rt_hip.h: "asynchronous on `stream`"), tolerance 0.

The rest of the suite passes stream = NULL or torch's current stream — both the legacy null stream — where a launch, a fill or a copy
inside a multi-launch call that was handed 0 or the context's own stream instead of `stream` changes nothing.  Here every call goes
through tests/stream_harness.py: a non-blocking stream, poison in every input, a sentinel in every output, a calibrated delay and the
producer's copies in front of the call, the consumer's copies right behind it, and the blindness guard after every call that is not
listed below.  What is compared is what the suite already compares on the null stream, as uint32 words, against the same references:
oracle.render, tests/denoise_reference.py, reproject_reference.py, upsample_reference.py, adaptive_reference.py, tonemap_reference.py,
bloom_reference.py.  No kernel arithmetic is in question; the order is.

Frames are 37 x 23 unless a case says otherwise: ragged against 64 x 4, 32 x 8, 16 x 16 and the meter's runs of 4 pixels (851 pixels:
212 runs and a tail of 3), more than one workgroup of each kernel.  Every input condition a case leans on (a history count that is
neither 0 nor all, orphans, 3 bloom levels, a mask with both kinds of pixel) is asserted on the CPU reference before the device is asked.

A pass is whole chunks of 16 samples and starts on a multiple of 16 (rt_hip_render_pass_device refuses anything else but a last pass that
ends on the sample count): the smallest two passes onto one accumulator are 2 x 16, held to the 32-sample one-shot frame."""
import functools

import numpy as np
import pytest

import rt_amd
from oracle import binding as oracle
from rt_amd import capi
from tests import adaptive_masks as masks
from tests import adaptive_reference as adaptive_ref
from tests import bloom_reference as bloom_ref
from tests import denoise_reference as denoise_ref
from tests import reproject_reference as reproject_ref
from tests import stream_harness
from tests import temporal_cases
from tests import tonemap_reference as tonemap_ref
from tests import upsample_reference as upsample_ref
from tests.conftest import GOLDEN
from tests.stream_harness import Harness, Step, run
from tests.test_gpu_partition_sweep import gathered_words
from tests.test_gpu_progressive import field

pytestmark = pytest.mark.gpu

F32 = np.float32
W, H = 37, 23
LOW_W, LOW_H = 19, 12  # rt_hip_upsample_low_size(37, 23, 2)
P = W * H
SEED = 5
BVH, DEVICE_BUILD, BOXES = capi.RT_HIP_FLAG_BVH, capi.RT_HIP_FLAG_BVH_DEVICE_BUILD, capi.RT_HIP_FLAG_TRACE_BOXES
STOPPED, COUNT = adaptive_ref.STOPPED, adaptive_ref.COUNT

# Calls the header calls asynchronous that wait on the host BY DESIGN: held to their results only, and so is whatever follows them behind
# the same delay.  Each with the line that waits and the sentence of include/rt_hip.h (or of the code) that says so.
WAITS_BY_DESIGN = {
    "render_device with RT_HIP_FLAG_BVH_DEVICE_BUILD": "rt_amd/csrc/scene.hip:390 hipStreamSynchronize(stream) in build_bvh_on_device: rt_hip_render_device keeps stats, and `upload_ms` includes the build on frames that "
                                                       "keep stats (the call then waits for it) — include/rt_hip.h, RT_HIP_FLAG_BVH_DEVICE_BUILD",
    "stats behind adaptive_pass_device": "rt_amd/csrc/render.hip:322 hipEventSynchronize(ctx->counters_copied) in fetch_member_stats: reading the counters is what waits, not the pass",
    "a call that grows a context's scratch": "rt_amd/csrc/internal.hpp:98 hipFree(ptr) in device_buffer::reserve: hipFree waits for the device, which is what keeps the block alive for the kernels still queued on it",
}


def words(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype != np.uint32 else a


def assert_same(h, buffer, want, what):
    got, want = h.got(buffer), words(want)
    got = got.reshape(-1)[: want.size].reshape(want.shape)
    differing = got != want
    assert not differing.any(), f"{h.what}: {what}: {int(differing.sum())} of {differing.size} words differ from the reference, first at {tuple(int(v) for v in np.argwhere(differing)[0])}: {got[differing][0]:08x} for {want[differing][0]:08x}"


@pytest.fixture(scope="module")
def mine():
    """A context of this file's own: what its stream was last is nobody else's business."""
    with rt_amd.HipRayTracer(device=0) as t:
        yield t


def basic(spp, width=W, height=H):
    return rt_amd.Scene.named("basic").set_sampling(spp).describe(width, height)


def noise(shape, seed, low=0.0, high=1.2):
    return np.random.default_rng(seed).uniform(low, high, size=shape).astype(F32)


# ---- a. one test per entry point ---------------------------------------------------------------------------------------------------------
def test_render_device_with_and_without_the_float_mean(mine):
    pod = basic(4)
    mine.upload(pod)
    want = [oracle.render(pod, W, H, seed=seed) for seed in (SEED, SEED + 1)]
    h = Harness("render_device")
    rows = rt_amd.padded_local_rows(H, 1)
    rgba, rgb, packed_only = h.sink((rows, W)), h.sink((rows, W, 3)), h.sink((rows, W))
    run([Step(h, lambda: mine.render_device(W, H, rgba.data_ptr(), seed=SEED, d_rgb_f32=rgb.data_ptr(), stream=h.handle), "with d_rgb_f32"),
         Step(h, lambda: mine.render_device(W, H, packed_only.data_ptr(), seed=SEED + 1, stream=h.handle), "without d_rgb_f32")])
    assert_same(h, rgba, want[0][0], "packed pixels")
    assert_same(h, rgb, want[0][1], "float mean")
    assert_same(h, packed_only, want[1][0], "packed pixels alone")


def test_render_device_with_the_hierarchy_built_on_the_frames_stream(mine):
    """48 spheres: the device builder's launches and the frame ride one stream.  The tree is made stale in front of every round (a frame
    through the host's tree: the cached tree remembers its builder), so the measured call really builds.  It waits: WAITS_BY_DESIGN."""
    pod = field(48, 1, 4, 31)
    mine.upload(pod)
    want_rgba, want_rgb, want_stats = oracle.render(pod, W, H, seed=SEED)
    h = Harness("render_device, device BVH build")
    rgba, rgb, other = h.sink((H, W)), h.sink((H, W, 3)), h.sink((H, W), read=False)

    def stale():
        mine.render_device(W, H, other.data_ptr(), seed=SEED, flags=BVH, stream=h.handle)
        h.stream.synchronize()

    run([Step(h, lambda: mine.render_device(W, H, rgba.data_ptr(), seed=SEED, flags=BVH | DEVICE_BUILD, d_rgb_f32=rgb.data_ptr(), stream=h.handle), "build + frame", WAITS_BY_DESIGN["render_device with RT_HIP_FLAG_BVH_DEVICE_BUILD"])],
        settle=stale)
    assert_same(h, rgba, want_rgba, "packed pixels")
    assert_same(h, rgb, want_rgb, "float mean")
    stats = mine.stats()
    assert stats["kernel"] == "bvh" and stats["segments"] == want_stats["segments"], stats


def test_render_pass_device_two_passes_back_to_back(mine):
    pod = basic(32)
    mine.upload(pod)
    want_rgba, want_rgb, _ = oracle.render(pod, W, H, seed=SEED)
    h = Harness("render_pass_device")
    rows = rt_amd.padded_local_rows(H, 1)
    accum, rgba, rgb = h.sink((rows, W, 3), read=False), h.sink((rows, W)), h.sink((rows, W, 3))  # (the first pass reads nothing of the accumulator)
    one_pass = lambda first: lambda: mine.render_pass_device(W, H, first, 16, accum.data_ptr(), rgba.data_ptr(), seed=SEED, d_rgb_f32=rgb.data_ptr(), stream=h.handle)  # noqa: E731
    run([Step(h, one_pass(0), "samples 0..16"), Step(h, one_pass(16), "samples 16..32")])
    assert_same(h, rgba, want_rgba, "packed pixels after 32 samples")
    assert_same(h, rgb, want_rgb, "float mean after 32 samples")


def test_assemble_device_three_ranks_stripes(mine):
    width, height, world, stripe = 37, 29, 3, 8
    gathered, want = gathered_words(width, height, world, stripe)
    poison = np.roll(gathered, 1, axis=0) ^ np.uint32(0x00000400)  # other ranks' words, other columns
    h = Harness("assemble_device")
    d_gathered, frame = h.feed(gathered, poison), h.sink((height, width))
    run([Step(h, lambda: mine.assemble_device(width, height, world, stripe, d_gathered.data_ptr(), frame.data_ptr(), h.handle), "assemble")])
    assert_same(h, frame, want, "the frame")


@pytest.mark.parametrize("name", ["basic", "boxes_toml_with_the_flag"])
def test_guide_device(mine, name):
    pod = basic(4) if name == "basic" else rt_amd.Scene.load(GOLDEN / "scenes" / "boxes.toml").describe(W, H)
    flags = 0 if name == "basic" else BOXES
    want = denoise_ref.compose_guide(pod, W, H, boxes=bool(flags))
    if flags:
        assert (reproject_ref.ids_of(want) > pod.n_spheres + pod.n_planes).any()  # a box in sight
    mine.upload(pod)
    h = Harness(f"guide_device, {name}")
    guide = h.sink((H, W, 8))
    run([Step(h, lambda: mine.guide_device(W, H, guide.data_ptr(), flags=flags, stream=h.handle), "guide")])
    assert_same(h, guide, want, "all 8 words")


def guides(height, width, seed):
    return upsample_ref.random_guide(np.random.default_rng(seed), height, width)


@pytest.mark.parametrize("iterations", [1, 2, 3, 6])  # both LDS builds, the gather build, both blocks of the ping-pong
def test_denoise_device(mine, iterations):
    image, guide, p = noise((H, W, 3), 10 + iterations), guides(H, W, 20 + iterations), denoise_ref.params(iterations=iterations)
    want_rgb, want_rgba = denoise_ref.filter(image, guide, p)
    h = Harness(f"denoise_device, {iterations} iterations")
    d_in, d_guide = h.feed(image, noise((H, W, 3), 110 + iterations)), h.feed(guide, guides(H, W, 120 + iterations))
    out, rgba = h.sink((H, W, 3)), h.sink((H, W))
    run([Step(h, lambda: mine.denoise_device(W, H, d_in.data_ptr(), d_guide.data_ptr(), p, out.data_ptr(), rgba.data_ptr(), stream=h.handle), "filter")])
    assert_same(h, out, want_rgb, "float frame")
    assert_same(h, rgba, want_rgba, "packed pixels")


def test_reproject_device_without_and_with_a_history(mine):
    pods, case_guides, _ = temporal_cases.case("basic:dolly", W, H)
    current = [temporal_cases.oracle_mean(pods[k], W, H, 3 + k) for k in (0, 1)]
    first = reproject_ref.frame(pods[0], case_guides[0], current[0], 16)
    second = reproject_ref.frame(pods[1], case_guides[1], current[1], 16, reproject_ref.matrix_of(pods[0]), first[0], first[1])
    assert first[2] == 0 and 0 < second[2] < P, (first[2], second[2])  # history was found, and not everywhere
    # frame 0: both history pointers NULL
    mine.upload(pods[0])
    h = Harness("reproject_device, no history")
    d_guide, d_rgb = h.feed(case_guides[0], case_guides[1]), h.feed(current[0], current[1])
    out, record, found = h.sink((H, W, 3)), h.sink((H, W, 8)), h.sink(1)
    run([Step(h, lambda: mine.reproject_device(W, H, None, d_guide.data_ptr(), d_rgb.data_ptr(), 16, None, None, None, out.data_ptr(), record.data_ptr(), found.data_ptr(), stream=h.handle), "frame 0")])
    assert_same(h, out, first[0], "colour"), assert_same(h, record, first[1], "record")
    assert int(h.got(found)[0]) == first[2]
    # frame 1: the device's own output of frame 0 is the history, under the moved camera
    history_rgb, history_record = h.got(out).view(F32).reshape(H, W, 3), h.got(record).view(F32).reshape(H, W, 8)
    other = reproject_ref.frame(pods[1], case_guides[1], current[1], 16)  # (another valid history: the poison)
    mine.upload(pods[1])
    h = Harness("reproject_device, with a history")
    d_guide, d_rgb = h.feed(case_guides[1], case_guides[0]), h.feed(current[1], current[0])
    d_prev_rgb, d_prev_record = h.feed(history_rgb, other[0]), h.feed(history_record, other[1])
    out, record, found = h.sink((H, W, 3)), h.sink((H, W, 8)), h.sink(1)
    run([Step(h, lambda: mine.reproject_device(W, H, reproject_ref.matrix_of(pods[0]), d_guide.data_ptr(), d_rgb.data_ptr(), 16, d_prev_rgb.data_ptr(), d_prev_record.data_ptr(), None, out.data_ptr(), record.data_ptr(), found.data_ptr(),
                                               stream=h.handle), "frame 1")])
    assert_same(h, out, second[0], "colour"), assert_same(h, record, second[1], "record")
    assert int(h.got(found)[0]) == second[2]


def test_upsample_device_by_2(mine):
    assert upsample_ref.low_size(W, H, 2)[2:] == (LOW_W, LOW_H)
    low, guide_low, guide_full = noise((LOW_H, LOW_W, 3), 1), guides(LOW_H, LOW_W, 2), guides(H, W, 3)
    want_rgb, want_rgba, want_orphans = upsample_ref.frame(low, guide_low, guide_full)
    assert 0 < want_orphans < P, want_orphans
    h = Harness("upsample_device")
    d_low, d_guide_low, d_guide_full = h.feed(low, noise((LOW_H, LOW_W, 3), 101)), h.feed(guide_low, guides(LOW_H, LOW_W, 102)), h.feed(guide_full, guides(H, W, 103))
    out, rgba, orphans = h.sink((H, W, 3)), h.sink((H, W)), h.sink(1)
    run([Step(h, lambda: mine.upsample_device(W, H, LOW_W, LOW_H, d_low.data_ptr(), d_guide_low.data_ptr(), d_guide_full.data_ptr(), None, out.data_ptr(), rgba.data_ptr(), orphans.data_ptr(), stream=h.handle), "upsample")])
    assert_same(h, out, want_rgb, "float frame"), assert_same(h, rgba, want_rgba, "packed pixels")
    assert int(h.got(orphans)[0]) == want_orphans


def update_inputs(width, height, seed):
    """Two passes of 16 for the update kernel alone, in the manner of tests/test_gpu_adaptive_masks.py: per pass (accum, pass_sum); three
    pixels in ten are noisy (their two pass sums disagree), the others agree with themselves."""
    rng = np.random.default_rng(seed)
    level = rng.uniform(0.1, 1.0, size=(height, width, 3))
    noisy = rng.random((height, width)) < 0.3
    sums = [(np.where(noisy[..., None], factor, 1.0) * level * 16).astype(F32) for factor in (0.1, 1.9)]
    return [(sums[0], sums[0]), ((sums[0] + sums[1]).astype(F32), sums[1])]


def update_buffers(h, width, height, accum, pass_sum, moments, state, poison):
    """The buffers of one rt_hip_adaptive_update_device call on `h`: moments and state are updated in place and read back."""
    return {"accum": h.feed(accum, poison["accum"]), "pass_sum": h.feed(pass_sum, poison["pass_sum"]), "moments": h.read(h.feed(moments, poison["moments"])), "state": h.read(h.feed(state, poison["state"])),
            "rgba": h.sink((height, width)), "rgb": h.sink((height, width, 3)), "active": h.sink(1)}


def update_call(tracer, h, width, height, first_pass, b):
    return lambda: tracer.adaptive_update_device(width, height, 16, first_pass, True, b["accum"].data_ptr(), b["pass_sum"].data_ptr(), b["moments"].data_ptr(), b["state"].data_ptr(), b["rgba"].data_ptr(), params=None,
                                                 d_rgb_out=b["rgb"].data_ptr(), d_active_pixels=b["active"].data_ptr(), stream=h.handle)


def assert_update(h, b, want, what):
    want_moments, want_state, want_rgba, want_rgb, want_active = want
    assert_same(h, b["state"], want_state, f"{what}: state words"), assert_same(h, b["moments"], want_moments, f"{what}: moments")
    assert_same(h, b["rgba"], want_rgba, f"{what}: packed pixels"), assert_same(h, b["rgb"], want_rgb, f"{what}: float mean")
    assert int(h.got(b["active"])[0]) == want_active, (what, int(h.got(b["active"])[0]), want_active)


def update_poison(width, height, seed):
    accum, pass_sum = update_inputs(width, height, seed)[1]
    return {"accum": accum, "pass_sum": pass_sum, "moments": noise((height, width, 2), seed, 0.1, 9.0), "state": np.where(np.random.default_rng(seed).random((height, width)) < 0.5, np.uint32(16) | STOPPED, np.uint32(16)).astype(np.uint32)}


def test_adaptive_update_device_a_first_and_a_second_step_under_a_constructed_mask(mine):
    passes = update_inputs(W, H, 7)
    blank_moments, blank_state = np.full((H, W, 2), np.nan, dtype=F32), np.full((H, W), 0xFFFFFFFF, dtype=np.uint32)  # (the first pass writes them and does not read them)
    first = adaptive_ref.step(*passes[0], blank_moments, blank_state, 16, True, True)
    mask = masks.mask("random_half", W, H, 3, 6)
    assert mask.any() and (~mask).any()  # both kinds of pixel
    masked = first[1] | np.where(mask, STOPPED, np.uint32(0))
    second = adaptive_ref.step(*passes[1], first[0], masked, 16, False, True)
    assert 0 < second[4] < P and np.array_equal(second[1][mask], masked[mask])  # some go on, some stop, the hand-stopped keep their words
    h = Harness("adaptive_update_device, first step")
    b = update_buffers(h, W, H, *passes[0], blank_moments, blank_state, update_poison(W, H, 107))
    run([Step(h, update_call(mine, h, W, H, True, b), "first pass")])
    assert_update(h, b, first, "first pass")
    h = Harness("adaptive_update_device, second step")
    b = update_buffers(h, W, H, *passes[1], first[0], masked, update_poison(W, H, 108))
    run([Step(h, update_call(mine, h, W, H, False, b), "second pass")])
    assert_update(h, b, second, "second pass")


def block_of(got, pixels, width, height):
    got = got.reshape(-1)
    return got[: 3 * pixels].reshape(height, width, 3), got[3 * pixels : 4 * pixels].reshape(height, width), got[4 * pixels : 7 * pixels].reshape(height, width, 3), got[7 * pixels :].reshape(height, width, 2)


def test_adaptive_pass_device_two_passes_and_the_stats_while_the_delay_is_pending(mine):
    """One pass, then — from a block of NaNs again — two passes back to back and rt_hip_stats_fetch behind them (it waits:
    WAITS_BY_DESIGN).  The second pass is replayed by the restatement from the first run's words and its own fold."""
    pod = basic(32)
    mine.upload(pod)
    at = {spp: oracle.render(basic(spp), W, H, seed=SEED) for spp in (16, 32)}

    def passes(h, count, with_stats):
        block, frame, mean, active = h.sink(9 * P), h.sink((H, W)), h.sink((H, W, 3)), h.sink(1)
        one = lambda first: lambda: mine.adaptive_pass_device(W, H, first, 16, block.data_ptr(), frame.data_ptr(), seed=SEED, d_rgb_f32=mean.data_ptr(), d_active_pixels=active.data_ptr(), stream=h.handle)  # noqa: E731
        steps = [Step(h, one(16 * k), f"pass {k}") for k in range(count)]
        if with_stats:
            steps.append(Step(h, mine.stats, "stats", WAITS_BY_DESIGN["stats behind adaptive_pass_device"]))
        return run(steps), block, frame, mean, active

    h0 = Harness("adaptive_pass_device, one pass")
    _, block, frame, mean, active = passes(h0, 1, False)
    accum0, state0, pass_sum0, moments0 = block_of(h0.got(block), P, W, H)
    want0 = adaptive_ref.step(accum0.view(F32), pass_sum0.view(F32), np.zeros((H, W, 2), dtype=F32), np.zeros((H, W), dtype=np.uint32), 16, True, True)
    assert np.array_equal(accum0, pass_sum0) and (state0 == 16).all() and np.array_equal(state0, want0[1]) and np.array_equal(moments0, words(want0[0]))
    assert_same(h0, frame, at[16][0], "the frame at 16"), assert_same(h0, mean, at[16][1], "the mean at 16")
    assert int(h0.got(active)[0]) == want0[4] == P  # (min_samples is two passes: nobody can stop)

    h1 = Harness("adaptive_pass_device, two passes + stats")
    results, block, frame, mean, active = passes(h1, 2, True)
    accum1, state1, pass_sum1, moments1 = block_of(h1.got(block), P, W, H)
    want1 = adaptive_ref.step(accum1.view(F32), pass_sum1.view(F32), moments0.view(F32), state0, 16, False, True)
    assert np.array_equal(state1, want1[1]), f"{int((state1 != want1[1]).sum())} state words differ from the restatement"
    assert np.array_equal(moments1, words(want1[0]))
    assert_same(h1, frame, want1[2], "the frame"), assert_same(h1, mean, want1[3], "the mean")
    assert ((state1 & COUNT) == 32).all()
    assert_same(h1, frame, at[32][0], "the frame at 32"), assert_same(h1, mean, at[32][1], "the mean at 32")
    assert int(h1.got(active)[0]) == want1[4] == int(((state1 & STOPPED) == 0).sum()) and 0 < want1[4] < P, want1[4]
    stats = results[-1]  # of the second pass: every pixel was active in it
    assert stats["primary_samples"] == P * 16 and stats["segments"] == at[32][2]["segments"] - at[16][2]["segments"], stats


@pytest.mark.parametrize("case", ["metered, in place", "manual exposure", "twice on one record"])
def test_tonemap_device(mine, case):
    frames = [tonemap_ref.noise(H, W, seed=31), tonemap_ref.noise(H, W, seed=32, low=-6.0, high=2.0)]
    bad_frames = [tonemap_ref.noise(H, W, seed=131), tonemap_ref.noise(H, W, seed=132, low=-3.0, high=9.0)]
    zeroed, bad_state = np.zeros(8, dtype=np.uint32), tonemap_ref.frame(bad_frames[0], tonemap_ref.params())[2]
    h = Harness(f"tonemap_device, {case}")
    state = h.read(h.feed(zeroed, bad_state))
    if case == "twice on one record":
        p = tonemap_ref.params(curve=tonemap_ref.REINHARD, adaptation=0.25)
        first = tonemap_ref.frame(frames[0], p)
        second = tonemap_ref.frame(frames[1], p, first[2])
        assert tonemap_ref.info_of(second[2])["exposure"] != tonemap_ref.info_of(second[2])["target"]  # the second call eases from the first
        d_in = [h.feed(frames[k], bad_frames[k]) for k in (0, 1)]
        out, rgba = [h.sink((H, W, 3)) for _ in (0, 1)], [h.sink((H, W)) for _ in (0, 1)]
        one = lambda k: lambda: mine.tonemap_device(W, H, d_in[k].data_ptr(), state.data_ptr(), p, out[k].data_ptr(), rgba[k].data_ptr(), stream=h.handle)  # noqa: E731
        run([Step(h, one(0), "first frame"), Step(h, one(1), "second frame")])
        for k, want in enumerate((first, second)):
            assert_same(h, out[k], want[0], f"float frame {k}"), assert_same(h, rgba[k], want[1], f"packed pixels {k}")
        assert_same(h, state, second[2], "all 8 words of the record")
        return
    p = tonemap_ref.params(curve=tonemap_ref.ACES) if case == "metered, in place" else tonemap_ref.params(curve=tonemap_ref.REINHARD, exposure=0.5)
    want_rgb, want_rgba, want_state = tonemap_ref.frame(frames[0], p)
    d_in, rgba = h.read(h.feed(frames[0], bad_frames[0])), h.sink((H, W))
    run([Step(h, lambda: mine.tonemap_device(W, H, d_in.data_ptr(), state.data_ptr(), p, d_in.data_ptr(), rgba.data_ptr(), stream=h.handle), "tone map")])
    assert_same(h, d_in, want_rgb, "float frame, in place"), assert_same(h, rgba, want_rgba, "packed pixels")
    assert_same(h, state, want_state, "all 8 words of the record")
    if case == "manual exposure":
        assert tonemap_ref.info_of(want_state) == {"exposure": 0.5, "target": 0.5, "counted": 0, "skipped": 0, "kept": 0, "mean_q8": 0}


@pytest.mark.parametrize("in_place", [True, False], ids=["in place", "with d_layer_out"])
def test_bloom_device(mine, in_place):
    width, height = 70, 41
    p = bloom_ref.params()
    assert bloom_ref.plan(width, height, p)["levels"] >= 3
    rgb = bloom_ref.noise(height, width, seed=51)
    want_out, want_layer = bloom_ref.frame(rgb, p)
    h = Harness(f"bloom_device, {'in place' if in_place else 'with d_layer_out'}")
    d_in = h.feed(rgb, bloom_ref.noise(height, width, seed=151))
    out, layer = (h.read(d_in), None) if in_place else (h.sink((height, width, 3)), h.sink((height, width, 3)))
    run([Step(h, lambda: mine.bloom_device(width, height, d_in.data_ptr(), p, out.data_ptr(), layer.data_ptr() if layer is not None else None, stream=h.handle), "bloom")])
    assert_same(h, out, want_out, "the frame")
    if layer is not None:
        assert_same(h, layer, want_layer, "the glow layer")


# ---- b. the chain ------------------------------------------------------------------------------------------------------------------------
CAMERAS = [((0.0, 1.0, 3.0), (0.0, 0.0, -1.0)), ((0.11, 1.02, 2.93), (0.0, 0.0, -1.0))]  # basic.toml's own camera, then a dolly
CHAIN_TONEMAP = dict(curve=tonemap_ref.ACES, adaptation=0.5)
CHAIN_UPSAMPLE = dict(min_weight=0.1)  # (the default threshold leaves frame 1 without an orphan: a counter of 0 says nothing about its clear)


@functools.lru_cache(maxsize=None)
def chain_reference(k):
    """Frame k of the chain on the CPU: every intermediate, from the references alone (computed once, read-only)."""
    pod = temporal_cases.toml_scene("basic", W, H, *CAMERAS[k], spp=32)
    low_rgba, low_mean, _ = oracle.render(pod, LOW_W, LOW_H, seed=SEED + k)
    guide_low, guide_full = denoise_ref.compose_guide(pod, LOW_W, LOW_H), denoise_ref.compose_guide(pod, W, H)
    filtered, _ = denoise_ref.filter(low_mean, guide_low, denoise_ref.params(iterations=3))
    up, _, orphans = upsample_ref.frame(filtered, guide_low, guide_full, upsample_ref.params(**CHAIN_UPSAMPLE))
    previous = chain_reference(k - 1) if k else None
    history = (reproject_ref.matrix_of(previous["pod"]), previous["blended"], previous["record"]) if k else (None, None, None)
    blended, record, found = reproject_ref.frame(pod, guide_full, up, 32, *history)
    bloomed, _ = bloom_ref.frame(blended, bloom_ref.params())
    state_before = previous["state"] if k else np.zeros(8, dtype=np.uint32)
    _, packed, state = tonemap_ref.frame(bloomed, tonemap_ref.params(**CHAIN_TONEMAP), state_before)
    out = {"pod": pod, "low_rgba": low_rgba, "low_mean": low_mean, "guide_low": guide_low, "guide_full": guide_full, "filtered": filtered, "up": up, "orphans": orphans, "blended": blended, "record": record, "found": found,
           "bloomed": bloomed, "packed": packed, "state": state, "state_before": state_before}
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def test_the_whole_post_process_chain_on_one_stream_without_a_host_synchronisation(mine):
    """render passes (low) -> guides (low, full) -> filter (low) -> upsample -> reproject -> bloom in place -> tone map, one delay in front
    and nothing but enqueues until the readback; run for a first camera (no history) and then, with that run's own device results as the
    history and the exposure record, for a moved one."""
    want = [chain_reference(0), chain_reference(1)]
    assert 0 < want[0]["orphans"] < P and 0 < want[1]["orphans"] < P and 0 < want[1]["found"] < P, (want[0]["orphans"], want[1]["orphans"], want[1]["found"])
    history = None
    for k in (0, 1):
        w = want[k]
        mine.upload(w["pod"])
        h = Harness(f"the chain, frame {k}")
        rows = rt_amd.padded_local_rows(LOW_H, 1)
        accum, low_rgba, low_mean = h.sink((rows, LOW_W, 3), read=False), h.sink((rows, LOW_W)), h.sink((rows, LOW_W, 3))
        guide_low, guide_full, filtered, up, orphans = h.sink((LOW_H, LOW_W, 8)), h.sink((H, W, 8)), h.sink((LOW_H, LOW_W, 3)), h.sink((H, W, 3)), h.sink(1)
        blended, record, found, packed = h.sink((H, W, 3), read=False), h.sink((H, W, 8)), h.sink(1), h.sink((H, W))
        h.read(blended, key="blended")  # (bloom then works in place on it: the consumer's copy goes in between)
        bloomed = h.read(blended)
        if k:
            other = want[0]
            prev_rgb, prev_record = h.feed(history[0], np.roll(other["blended"], 5, axis=1)), h.feed(history[1], np.roll(other["record"], 5, axis=1))
        state = h.read(h.feed(history[2] if k else w["state_before"], tonemap_ref.frame(tonemap_ref.noise(H, W, seed=61 + k))[2]))
        matrix = reproject_ref.matrix_of(want[0]["pod"]) if k else None
        p_filter, p_upsample, p_tonemap = denoise_ref.params(iterations=3), upsample_ref.params(**CHAIN_UPSAMPLE), tonemap_ref.params(**CHAIN_TONEMAP)

        def chain():
            s = h.handle
            for first in (0, 16):
                mine.render_pass_device(LOW_W, LOW_H, first, 16, accum.data_ptr(), low_rgba.data_ptr(), seed=SEED + k, d_rgb_f32=low_mean.data_ptr(), stream=s)
            mine.guide_device(LOW_W, LOW_H, guide_low.data_ptr(), stream=s)
            mine.guide_device(W, H, guide_full.data_ptr(), stream=s)
            mine.denoise_device(LOW_W, LOW_H, low_mean.data_ptr(), guide_low.data_ptr(), p_filter, filtered.data_ptr(), None, stream=s)
            mine.upsample_device(W, H, LOW_W, LOW_H, filtered.data_ptr(), guide_low.data_ptr(), guide_full.data_ptr(), p_upsample, up.data_ptr(), None, orphans.data_ptr(), stream=s)
            mine.reproject_device(W, H, matrix, guide_full.data_ptr(), up.data_ptr(), 32, prev_rgb.data_ptr() if k else None, prev_record.data_ptr() if k else None, None, blended.data_ptr(), record.data_ptr(), found.data_ptr(), stream=s)
            h.snap("blended")
            mine.bloom_device(W, H, blended.data_ptr(), None, blended.data_ptr(), None, stream=s)
            mine.tonemap_device(W, H, blended.data_ptr(), state.data_ptr(), p_tonemap, None, packed.data_ptr(), stream=s)

        run([Step(h, chain, "the nine calls")])
        got_blended = h.got("blended")
        what = f"frame {k}"
        assert_same(h, low_rgba, w["low_rgba"], f"{what}: the low packed frame"), assert_same(h, low_mean, w["low_mean"], f"{what}: the low mean after 2 x 16 samples")
        assert_same(h, guide_low, w["guide_low"], f"{what}: the low guide"), assert_same(h, guide_full, w["guide_full"], f"{what}: the full guide")
        assert_same(h, filtered, w["filtered"], f"{what}: the filtered low mean"), assert_same(h, up, w["up"], f"{what}: the upsampled frame")
        assert int(h.got(orphans)[0]) == w["orphans"] and int(h.got(found)[0]) == w["found"], (what, int(h.got(orphans)[0]), w["orphans"], int(h.got(found)[0]), w["found"])
        assert np.array_equal(got_blended, words(w["blended"])), f"{what}: the reprojected frame differs in {int((got_blended != words(w['blended'])).sum())} words"
        assert_same(h, record, w["record"], f"{what}: the record"), assert_same(h, bloomed, w["bloomed"], f"{what}: the bloomed frame")
        assert_same(h, packed, w["packed"], f"{what}: the final packed frame"), assert_same(h, state, w["state"], f"{what}: the tone map's record")
        history = (got_blended.view(F32).reshape(H, W, 3), h.got(record).view(F32).reshape(H, W, 8), h.got(state))


# ---- c. scratch that grows with work in flight -----------------------------------------------------------------------------------------------
SMALL, LARGE = (5, 3), (W, H)


def growth_steps(h, tracer, which, buffers):
    """The small and then the large call of `which` on `tracer`, over `buffers` (made once: the warm-up rounds use the same ones on a
    context of their own)."""
    steps = []
    for size, b, label, waits in zip((SMALL, LARGE), buffers, ("5 x 3", "37 x 23"), (None, WAITS_BY_DESIGN["a call that grows a context's scratch"])):
        width, height = size
        if which == "denoise":
            call = lambda width=width, height=height, b=b: tracer.denoise_device(width, height, b["in"].data_ptr(), b["guide"].data_ptr(), b["p"], b["out"].data_ptr(), b["rgba"].data_ptr(), stream=h.handle)  # noqa: E731
        elif which == "bloom":
            call = lambda width=width, height=height, b=b: tracer.bloom_device(width, height, b["in"].data_ptr(), b["p"], b["out"].data_ptr(), b["layer"].data_ptr(), stream=h.handle)  # noqa: E731
        else:
            call = update_call(tracer, h, width, height, True, b)
        steps.append(Step(h, call, label, waits))
    return steps


@pytest.mark.parametrize("which", ["denoise", "bloom", "adaptive_update"])
def test_a_contexts_scratch_grows_while_the_call_before_is_still_queued(which):
    """A fresh context: the 5 x 3 call reserves a small block, the 37 x 23 call behind it — the small one's kernels have not started —
    frees it and reserves a larger one.  The second call may wait (WAITS_BY_DESIGN); both results are the references'."""
    h = Harness(f"growing scratch, {which}")
    buffers, wants = [], []
    for n, (width, height) in enumerate((SMALL, LARGE)):
        if which == "denoise":
            image, guide, p = noise((height, width, 3), 70 + n), guides(height, width, 72 + n), denoise_ref.params(iterations=3)
            wants.append(denoise_ref.filter(image, guide, p))
            buffers.append({"in": h.feed(image, noise((height, width, 3), 170 + n)), "guide": h.feed(guide, guides(height, width, 172 + n)), "p": p, "out": h.sink((height, width, 3)), "rgba": h.sink((height, width))})
        elif which == "bloom":
            rgb, p = bloom_ref.noise(height, width, seed=74 + n), bloom_ref.params(levels=8)
            wants.append(bloom_ref.frame(rgb, p))
            buffers.append({"in": h.feed(rgb, bloom_ref.noise(height, width, seed=174 + n)), "p": p, "out": h.sink((height, width, 3)), "layer": h.sink((height, width, 3))})
        else:
            accum, pass_sum = update_inputs(width, height, 76 + n)[0]
            blank_moments, blank_state = np.full((height, width, 2), np.nan, dtype=F32), np.full((height, width), 0xFFFFFFFF, dtype=np.uint32)
            wants.append(adaptive_ref.step(accum, pass_sum, blank_moments, blank_state, 16, True, True))
            buffers.append(update_buffers(h, width, height, accum, pass_sum, blank_moments, blank_state, update_poison(width, height, 176 + n)))
    with rt_amd.HipRayTracer(device=0) as warm, rt_amd.HipRayTracer(device=0) as fresh:
        run(growth_steps(h, fresh, which, buffers), warm_steps=growth_steps(h, warm, which, buffers))
    for (width, height), b, want in zip((SMALL, LARGE), buffers, wants):
        what = f"{width} x {height}"
        if which == "denoise":
            assert_same(h, b["out"], want[0], f"{what}: float frame"), assert_same(h, b["rgba"], want[1], f"{what}: packed pixels")
        elif which == "bloom":
            assert_same(h, b["out"], want[0], f"{what}: the frame"), assert_same(h, b["layer"], want[1], f"{what}: the glow layer")
        else:
            assert_update(h, b, want, what)


# ---- d. two contexts, two streams, concurrently ------------------------------------------------------------------------------------------------
def test_two_contexts_on_two_streams_interleaved_each_get_their_own_results():
    """Scratch and state are per context: calls of A and B alternate on the host, each behind its own stream's delay, on different inputs."""
    with rt_amd.HipRayTracer(device=0) as a, rt_amd.HipRayTracer(device=0) as b:
        sides, steps_of = [], []
        for n, tracer in enumerate((a, b)):
            h = Harness(f"two contexts, {'AB'[n]}")
            image, guide, p_filter = noise((H, W, 3), 80 + n), guides(H, W, 82 + n), denoise_ref.params(iterations=3)
            hdr, p_tonemap = tonemap_ref.noise(H, W, seed=84 + n), tonemap_ref.params(curve=tonemap_ref.CURVES[1 + n])
            glow, p_bloom = bloom_ref.noise(41, 70, seed=86 + n), bloom_ref.params(levels=3 + n)
            d = {"image": h.feed(image, noise((H, W, 3), 180 + n)), "guide": h.feed(guide, guides(H, W, 182 + n)), "filtered": h.sink((H, W, 3)), "filtered_rgba": h.sink((H, W)),
                 "hdr": h.feed(hdr, tonemap_ref.noise(H, W, seed=184 + n)), "state": h.read(h.feed(np.zeros(8, dtype=np.uint32), tonemap_ref.frame(glow[:H, :W])[2])), "mapped": h.sink((H, W, 3)), "mapped_rgba": h.sink((H, W)),
                 "glow": h.feed(glow, bloom_ref.noise(41, 70, seed=186 + n)), "bloomed": h.sink((41, 70, 3)), "layer": h.sink((41, 70, 3))}
            sides.append((h, d, denoise_ref.filter(image, guide, p_filter), tonemap_ref.frame(hdr, p_tonemap), bloom_ref.frame(glow, p_bloom)))
            steps_of.append([
                Step(h, lambda t=tracer, h=h, d=d, p=p_filter: t.denoise_device(W, H, d["image"].data_ptr(), d["guide"].data_ptr(), p, d["filtered"].data_ptr(), d["filtered_rgba"].data_ptr(), stream=h.handle), "denoise"),
                Step(h, lambda t=tracer, h=h, d=d, p=p_tonemap: t.tonemap_device(W, H, d["hdr"].data_ptr(), d["state"].data_ptr(), p, d["mapped"].data_ptr(), d["mapped_rgba"].data_ptr(), stream=h.handle), "tonemap"),
                Step(h, lambda t=tracer, h=h, d=d, p=p_bloom: t.bloom_device(70, 41, d["glow"].data_ptr(), p, d["bloomed"].data_ptr(), d["layer"].data_ptr(), stream=h.handle), "bloom"),
            ])
        run([step for pair in zip(*steps_of) for step in pair])  # A, B, A, B, A, B
        for h, d, filtered, mapped, bloomed in sides:
            assert_same(h, d["filtered"], filtered[0], "filtered frame"), assert_same(h, d["filtered_rgba"], filtered[1], "filtered pixels")
            assert_same(h, d["mapped"], mapped[0], "mapped frame"), assert_same(h, d["mapped_rgba"], mapped[1], "mapped pixels"), assert_same(h, d["state"], mapped[2], "the record")
            assert_same(h, d["bloomed"], bloomed[0], "bloomed frame"), assert_same(h, d["layer"], bloomed[1], "glow layer")


# ---- the session's figures -----------------------------------------------------------------------------------------------------------------
def test_the_calibration_and_every_guard_of_this_session_are_on_record():
    """Last in the file: prints what profiles/r31/README.md records (pytest -s, or the captured output of a failure)."""
    stream_harness.spin_rate()
    print(stream_harness.report())
    assert all(f["delay_measured_ms"] >= stream_harness.MARGIN * f["host_ms"] or f["delay_asked_ms"] == stream_harness.MAX_DELAY_MS for f in stream_harness.FIGURES), stream_harness.report()
