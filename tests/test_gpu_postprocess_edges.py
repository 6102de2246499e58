"""The post-process kernels at every frame size around their tiles, in guarded buffers, tolerance 0.

Each of these kernels runs per-pixel text that the CPU restatement runs too (`*_rules.hpp`), so what is left for a kernel to get wrong is
HOW A TAP REACHES THE RULE — the LDS tile and its halo, the clip of the staged span, `alive`, the ring of verdicts, the grid stride, the
per-wave counts — and WHERE IT WRITES.  The first is a function of the frame size modulo the tile, so the sizes below come from the
tile geometry, not from a hand: along x every width from 1 to 2 Tw + h + 1 at the height Th + 1, along y every height from 1 to
2 Th + h + 1 at the width Tw + 1, and the cross {1, Tw - 1, Tw, Tw + 1, 2 Tw} x {1, Th - 1, Th, Th + 1, 2 Th}; for a linear kernel every
pixel count from 1 to 2 x 256 + 8 as n x 1 and {1, 63, 64, 65, 255, 256, 257, 513} as 1 x n.  The second is what tests/guarded.py is for:
every output of every call lies between sentinel bands that are checked, every input between NaN bands, every one-word count in a block
of its own, pre-set to a non-zero value.

The geometry, as the sources stand (h: how far the staged tile reaches past the tile, both sides together):

| kernel (entry point)                                            | tile    | h | source                                                        |
|-----------------------------------------------------------------|---------|---|---------------------------------------------------------------|
| guide_frame (rt_hip_guide_device)                               | 64 x 4  | 0 | denoise.hip:44-46 (64 lanes a row, block_threads / 64 rows)   |
| atrous_pass<1>, <2> (rt_hip_denoise_device, iterations 1, 2)    | 32 x 8  | 8 | denoise.hip:91 (tile), :105 (halo = 2 STEP a side: 2, then 4) |
| atrous_pass<0> (iterations 3 .. 6: gathered taps)               | 32 x 8  | - | denoise.hip:129-136                                           |
| finish_frame (iterations 0)                                     | 256     |   | denoise.hip:154-155                                           |
| reproject_frame (rt_hip_reproject_device)                       | 32 x 8  | 0 | temporal.hip:41, :53-54, :79-81 (the per-wave count)          |
| upsample_frame (rt_hip_upsample_device)                         | 16 x 16 | 1 | upsample.hip:43, :55-58 (x_last, lo / hi, span at most 17)    |
| adaptive_update (rt_hip_adaptive_update_device)                 | 16 x 16 | 2 | adaptive.hip:30-32 (ring of 68), :66-83, :113-130             |
| luminance_histogram, tonemap_frame (rt_hip_tonemap_device)      | 256     |   | tonemap.hip:58-75 (runs of 4, the tail, per-wave bins), :113  |
| bloom_down (rt_hip_bloom_device; bands: tests/test_gpu_bloom.py)| 16 x 16 |   | widths and heights 1 .. 35 only, levels = 8                   |

Left out: nothing of the guide's cross (its CPU side, a per-pixel Python composition, takes about two seconds in all)."""
import functools

import numpy as np
import pytest

import rt_amd
from tests import adaptive_reference as adaptive_ref
from tests import bloom_reference as bloom_ref
from tests import denoise_reference as denoise_ref
from tests import reproject_reference as reproject_ref
from tests import temporal_cases
from tests import tonemap_reference as tonemap_ref
from tests import upsample_reference as upsample_ref
from tests.guarded import COUNT_PRESET, SENTINEL, Arena, count_of

pytestmark = pytest.mark.gpu

F32 = np.float32
TILTED = ((0.2, 1.2, 3.0), (0.0, -0.15, -1.0))
STOPPED = adaptive_ref.STOPPED


def tiled_sizes(tw, th, h):
    """axis -> the (width, height) pairs of a kernel with tiles of tw x th whose staging reaches h pixels past them."""
    cross = [(w, hh) for w in (1, tw - 1, tw, tw + 1, 2 * tw) for hh in (1, th - 1, th, th + 1, 2 * th)]
    return {"x": [(w, th + 1) for w in range(1, 2 * tw + h + 2)], "y": [(tw + 1, hh) for hh in range(1, 2 * th + h + 2)], "cross": list(dict.fromkeys(cross))}


GUIDE_SIZES = tiled_sizes(64, 4, 0)
FILTER_SIZES = tiled_sizes(32, 8, 8)
REPROJECT_SIZES = tiled_sizes(32, 8, 0)
UPSAMPLE_SIZES = tiled_sizes(16, 16, 1)
ADAPTIVE_SIZES = tiled_sizes(16, 16, 2)
LINEAR_SIZES = {"row": [(n, 1) for n in range(1, 2 * 256 + 9)], "column": [(1, n) for n in (1, 63, 64, 65, 255, 256, 257, 513)]}
BLOOM_SIZES = {"x": [(w, 17) for w in range(1, 36)], "y": [(17, h) for h in range(1, 36)]}
AXES = ["x", "y", "cross"]


def test_the_sweeps_are_the_sizes_the_tiles_ask_for():
    assert (len(FILTER_SIZES["x"]), len(FILTER_SIZES["y"]), len(FILTER_SIZES["cross"])) == (73, 25, 25) and max(FILTER_SIZES["x"]) == (73, 9)
    assert GUIDE_SIZES["x"][-1] == (129, 5) and GUIDE_SIZES["y"][-1] == (65, 9) and (128, 8) in GUIDE_SIZES["cross"]
    assert REPROJECT_SIZES["x"][-1] == (65, 9) and (32, 8) in REPROJECT_SIZES["cross"] and (33, 9) in REPROJECT_SIZES["cross"]
    assert UPSAMPLE_SIZES["x"][-1] == (34, 17) and ADAPTIVE_SIZES["y"][-1] == (17, 35)
    assert len(LINEAR_SIZES["row"]) == 520 and LINEAR_SIZES["row"][-1] == (520, 1)
    assert SENTINEL == 0x7FC0BEEF and np.isnan(np.array([SENTINEL], dtype=np.uint32).view(F32)[0]) and COUNT_PRESET != 0  # (a NaN; counts start non-zero)


def device_of(tracer):
    return f"cuda:{tracer.device}"


def stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def poison(image, seed):
    """One NaN and one infinite pixel, where the frame has room for them beside a clean one."""
    height, width = image.shape[:2]
    if width * height >= 3:
        at = np.random.default_rng(seed).choice(width * height, size=2, replace=False)
        image.reshape(-1, 3)[at[0], 0] = np.nan
        image.reshape(-1, 3)[at[1], 2] = np.inf
    return image


# ---- the guide ----------------------------------------------------------------------------------------------------------------------
def guide_pod(scene, width, height):
    if scene == "basic tilted":
        return rt_amd.Scene.named("basic").set_sampling(16).set_camera(*TILTED).describe(width, height)
    from tests.test_gpu_denoise import planes_only

    return planes_only(width, height)


@pytest.mark.parametrize("axis", AXES)
@pytest.mark.parametrize("scene", ["basic tilted", "planes and sky"])
def test_the_guide(tracer, scene, axis):
    saw_sky = saw_hit = False
    for width, height in GUIDE_SIZES[axis]:
        pod = guide_pod(scene, width, height)
        want = denoise_ref.compose_guide(pod, width, height)
        ids = np.ascontiguousarray(want[..., 7]).view(np.uint32)
        saw_sky, saw_hit = saw_sky or bool((ids == 0).any()), saw_hit or bool((ids != 0).any())
        tracer.upload(pod)
        arena = Arena(device_of(tracer), width, 4)
        out = arena.output("d_guide", width * height, 8)
        tracer.guide_device(width, height, out.ptr, flags=0, stream=stream())
        arena.check()
        out.assert_is(want, f"{scene} {width}x{height}")
    assert saw_hit and (saw_sky or scene == "basic tilted")


# ---- the filter ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def filter_inputs(width, height):
    rng = np.random.default_rng(7000 * width + height)
    image = poison(rng.uniform(-0.2, 1.5, size=(height, width, 3)).astype(F32), width + height)
    return frozen(image, upsample_ref.random_guide(rng, height, width))


def filter_params(iterations):
    return denoise_ref.params(iterations=iterations, normal_squarings=3, sigma_colour=1.5, sigma_albedo=0.5, sigma_depth=0.2)


@functools.lru_cache(maxsize=None)
def filtered(width, height, iterations):
    image, guide = filter_inputs(width, height)
    return frozen(*denoise_ref.filter(image, guide, filter_params(iterations)))


def run_filter(tracer, width, height, iterations, tile_h, want_rgb=True, want_rgba=True):
    image, guide = filter_inputs(width, height)
    want = filtered(width, height, iterations)
    what = f"{width}x{height}, {iterations} iterations" + ("" if want_rgb and want_rgba else ", one output")
    arena = Arena(device_of(tracer), width, tile_h)
    d_in, d_guide = arena.input("d_rgb_in", image, 3), arena.input("d_guide", guide, 8)
    d_out = arena.output("d_rgb_out", width * height, 3) if want_rgb else None
    d_rgba = arena.output("d_rgba8_out", width * height, 1) if want_rgba else None
    tracer.denoise_device(width, height, d_in.ptr, d_guide.ptr, filter_params(iterations), d_out.ptr if want_rgb else None, d_rgba.ptr if want_rgba else None, stream=stream())
    arena.check()
    if want_rgb:
        d_out.assert_is(want[0], what)
    if want_rgba:
        d_rgba.assert_is(want[1], what)


@pytest.mark.parametrize("axis", AXES)
@pytest.mark.parametrize("iterations", [1, 2, 4])
def test_the_filter(tracer, iterations, axis):
    """1: atrous_pass<1> alone; 2: <1> then <2>; 4: two gathering steps more, whose taps at step 8 (16 pixels out) leave every swept
    frame on some side."""
    for width, height in FILTER_SIZES[axis]:
        run_filter(tracer, width, height, iterations, 8)
        if axis == "cross":
            run_filter(tracer, width, height, iterations, 8, want_rgba=False)
            run_filter(tracer, width, height, iterations, 8, want_rgb=False)


@pytest.mark.parametrize("axis", list(LINEAR_SIZES))
def test_the_filter_with_0_iterations_copies_and_packs(tracer, axis):
    for width, height in LINEAR_SIZES[axis]:
        run_filter(tracer, width, height, 0, 1)
    for width, height in LINEAR_SIZES["column"]:
        run_filter(tracer, width, height, 0, 1, want_rgba=False)
        run_filter(tracer, width, height, 0, 1, want_rgb=False)


# ---- reprojection -------------------------------------------------------------------------------------------------------------------
DOLLY = (0.11, 1.02, 2.93)  # tests/temporal_cases.py's dolly from basic.toml's camera


def run_reproject(tracer, pod, guide, rgb, prev, what):
    height, width = rgb.shape[:2]
    tracer.upload(pod)
    arena = Arena(device_of(tracer), width, 8)
    d_guide, d_rgb = arena.input("d_guide", guide, 8), arena.input("d_rgb_in", rgb, 3)
    d_prev_rgb, d_prev_record = (arena.input("d_prev_rgb", prev[1], 3), arena.input("d_prev_record", prev[2], 8)) if prev else (None, None)
    d_out, d_record, d_found = arena.output("d_rgb_out", width * height, 3), arena.output("d_record_out", width * height, 8), arena.count("d_pixels_with_history")
    tracer.reproject_device(width, height, prev[0] if prev else None, d_guide.ptr, d_rgb.ptr, 16, d_prev_rgb.ptr if prev else None, d_prev_record.ptr if prev else None, None, d_out.ptr, d_record.ptr, d_found.ptr, stream=stream())
    arena.check()
    want_rgb, want_record, want_found = reproject_ref.frame(pod, guide, rgb, 16, *(prev if prev else (None, None, None)))
    d_out.assert_is(want_rgb, what), d_record.assert_is(want_record, what)
    assert count_of(d_found) == want_found, (what, count_of(d_found), want_found)
    return want_rgb, want_record, want_found


@pytest.mark.parametrize("axis", AXES)
def test_reprojection(tracer, axis):
    """Frame 0 has no history and leaves a record; frame 1 meets it under the same camera, and under a small dolly.  The guide is data
    here: a random one (the rule takes the surface point from the centre ray and the guide's depth)."""
    for width, height in REPROJECT_SIZES[axis]:
        rng = np.random.default_rng(9000 * width + height)
        guide = upsample_ref.random_guide(rng, height, width)
        frames = [poison(rng.uniform(-0.2, 1.5, size=(height, width, 3)).astype(F32), k) for k in range(3)]
        rest, dolly = temporal_cases.toml_scene("basic", width, height), temporal_cases.toml_scene("basic", width, height, DOLLY)
        first = run_reproject(tracer, rest, guide, frames[0], None, f"{width}x{height} frame 0")
        assert first[2] == 0
        prev = (reproject_ref.matrix_of(rest), first[0], first[1])
        resting = run_reproject(tracer, rest, guide, frames[1], prev, f"{width}x{height} at rest")
        if (reproject_ref.ids_of(guide) != 0).any():
            assert resting[2] > 0, f"{width}x{height}: no pixel found its history under the camera that made it"
        run_reproject(tracer, dolly, guide, frames[2], prev, f"{width}x{height} after a dolly")


# ---- guided upsampling --------------------------------------------------------------------------------------------------------------
UPSAMPLE_PARAMS = {"defaults": {}, "wide, min_weight 1": dict(normal_squarings=0, sigma_albedo=5.0, sigma_depth=5.0, min_weight=1.0)}


def low_sizes(W, H):
    """w = W (the widest staged span), ceil(W / 2), ceil(W / 3) and one low pixel; the heights likewise."""
    return list(dict.fromkeys([(W, H), (-(-W // 2), -(-H // 2)), (-(-W // 3), -(-H // 3)), (1, 1)]))


def run_upsample(tracer, low, guide_low, guide_full, fields, what):
    h, w = low.shape[:2]
    H, W = guide_full.shape[:2]
    p = upsample_ref.params(**fields)
    arena = Arena(device_of(tracer), W, 16)
    d_low, d_guide_low, d_guide_full = arena.input("d_rgb_low", low, 3), arena.input("d_guide_low", guide_low, 8), arena.input("d_guide_full", guide_full, 8)
    d_out, d_rgba, d_orphans = arena.output("d_rgb_out", W * H, 3), arena.output("d_rgba8_out", W * H, 1), arena.count("d_orphans")
    tracer.upsample_device(W, H, w, h, d_low.ptr, d_guide_low.ptr, d_guide_full.ptr, p, d_out.ptr, d_rgba.ptr, d_orphans.ptr, stream=stream())
    arena.check()
    want_rgb, want_rgba, want_orphans = upsample_ref.frame(low, guide_low, guide_full, p)
    d_out.assert_is(want_rgb, what), d_rgba.assert_is(want_rgba, what)
    assert count_of(d_orphans) == want_orphans, (what, count_of(d_orphans), want_orphans)
    return want_orphans


@pytest.mark.parametrize("axis", AXES)
def test_upsampling(tracer, axis):
    orphans = guided = 0
    for W, H in UPSAMPLE_SIZES[axis]:
        for w, h in low_sizes(W, H):
            rng = np.random.default_rng(((W * 64 + H) * 64 + w) * 64 + h)
            low = poison(rng.uniform(-0.2, 1.5, size=(h, w, 3)).astype(F32), W + H)
            guide_low, guide_full = upsample_ref.random_guide(rng, h, w), upsample_ref.random_guide(rng, H, W)
            for name, fields in UPSAMPLE_PARAMS.items():
                n = run_upsample(tracer, low, guide_low, guide_full, fields, f"{W}x{H} from {w}x{h}, {name}")
                orphans, guided = orphans + n, guided + W * H - n
    assert orphans > 0 and guided > 0  # (both branches of the rule were met)


# ---- the adaptive update ------------------------------------------------------------------------------------------------------------
def run_update(tracer, accum, pass_sum, moments, state, n, first, whole, what):
    height, width = state.shape
    p = adaptive_ref.params()
    arena = Arena(device_of(tracer), width, 16)
    d_accum, d_pass_sum = arena.input("d_accum", accum, 3), arena.input("d_pass_sum", pass_sum, 3)
    d_moments, d_state = arena.inout("d_moments", moments, 2), arena.inout("d_state", state, 1)
    d_rgba, d_rgb, d_active = arena.output("d_rgba8_out", width * height, 1), arena.output("d_rgb_out", width * height, 3), arena.count("d_active_pixels")
    tracer.adaptive_update_device(width, height, n, first, whole, d_accum.ptr, d_pass_sum.ptr, d_moments.ptr, d_state.ptr, d_rgba.ptr, params=p, d_rgb_out=d_rgb.ptr, d_active_pixels=d_active.ptr, stream=stream())
    arena.check()
    want_moments, want_state, want_rgba, want_rgb, want_active = adaptive_ref.step(accum, pass_sum, moments, state, n, first, whole, p)
    d_state.assert_is(want_state, what, every_word_written=False), d_moments.assert_is(want_moments, what, every_word_written=False)
    d_rgba.assert_is(want_rgba, what), d_rgb.assert_is(want_rgb, what)
    assert count_of(d_active) == want_active == int(((want_state & STOPPED) == 0).sum()), (what, count_of(d_active), want_active)
    return want_moments, want_state


def five_steps(tracer, width, height):
    """tests/test_gpu_adaptive.py's sequence — a first pass, three whole passes, a short one — on a field of which 70 % is flat."""
    rng = np.random.default_rng(100 * width + height)
    flat = rng.random((height, width)) < 0.7
    level = rng.uniform(0.1, 1.0, size=(height, width, 3))
    accum = np.zeros((height, width, 3), dtype=F32)
    moments = np.full((height, width, 2), np.nan, dtype=F32)
    state = np.full((height, width), 0xFFFFFFFF, dtype=np.uint32)  # (the first pass writes them and does not read them)
    for k, (n, whole) in enumerate([(16, True), (16, True), (16, True), (16, True), (8, False)]):
        pass_sum = (np.where(flat[..., None], level, rng.uniform(0.0, 2.0, size=(height, width, 3))) * n).astype(F32)
        if k == 2:
            pass_sum[rng.random((height, width)) < 0.05] = np.nan  # a NaN never converges
        active = np.ones((height, width), dtype=bool) if k == 0 else (state & STOPPED) == 0
        with np.errstate(invalid="ignore"):
            accum = np.where(active[..., None], pass_sum if k == 0 else accum + pass_sum, accum).astype(F32)
        pass_sum[~active] = np.nan  # stale scratch: must not be read
        moments, state = run_update(tracer, accum, pass_sum, moments, state, n, k == 0, whole, f"{width}x{height} step {k}")
    return state


@pytest.mark.parametrize("axis", AXES)
def test_the_adaptive_update(tracer, axis):
    stopped = going = 0
    for width, height in ADAPTIVE_SIZES[axis]:
        state = five_steps(tracer, width, height)
        stopped, going = stopped + int(((state & STOPPED) != 0).sum()), going + int(((state & STOPPED) == 0).sum())
    assert stopped > 0 and going > 0


# corners and edge midpoints of the middle 16 x 16 tile of a 48 x 48 frame, and the pixel one beyond each, outwards: (x, y)
INSIDE = [(16, 16), (31, 16), (16, 31), (31, 31), (24, 16), (24, 31), (16, 24), (31, 24)]
BEYOND = [(15, 15), (32, 15), (15, 32), (32, 32), (24, 15), (24, 32), (15, 24), (32, 24)]


@pytest.mark.parametrize("x,y", INSIDE + BEYOND, ids=[f"{x},{y}" for x, y in INSIDE + BEYOND])
def test_one_unconverged_pixel_at_the_rim_of_a_tile_is_read_through_the_ring(tracer, x, y):
    """Pass sums of 0.1 n then 1.9 n times its level for the one pixel, n times theirs for all others (who converge at pass 2: two equal
    luminances have variance 0): after pass 2 exactly its 3 x 3 neighbourhood goes on, and that crosses one or two tile borders — the
    workgroups beside it know its verdict only through their ring, the corner entries included."""
    width = height = 48
    rng = np.random.default_rng(x * 64 + y)
    level = rng.uniform(0.1, 1.0, size=(height, width, 3))
    noisy = np.zeros((height, width), dtype=bool)
    noisy[y, x] = True
    accum = np.zeros((height, width, 3), dtype=F32)
    moments, state = np.full((height, width, 2), np.nan, dtype=F32), np.full((height, width), 0xFFFFFFFF, dtype=np.uint32)
    for k, factor in enumerate((0.1, 1.9)):
        pass_sum = (np.where(noisy[..., None], factor, 1.0) * level * 16).astype(F32)
        accum = (pass_sum if k == 0 else accum + pass_sum).astype(F32)
        moments, state = run_update(tracer, accum, pass_sum, moments, state, 16, k == 0, True, f"({x}, {y}) pass {k}")
    want = np.zeros((height, width), dtype=bool)
    want[y - 1 : y + 2, x - 1 : x + 2] = True
    going = (state & STOPPED) == 0
    assert np.array_equal(going, want), np.argwhere(going != want)[:8].tolist()
    assert len({(int(qx) // 16, int(qy) // 16) for qy, qx in np.argwhere(going)}) >= 2  # (the neighbourhood lies in more than one tile)


# ---- tone mapping -------------------------------------------------------------------------------------------------------------------
TONEMAP_PARAMS = {"metered, ACES": dict(curve=tonemap_ref.ACES), "manual exposure, Reinhard": dict(curve=tonemap_ref.REINHARD, exposure=0.37)}
IN_PLACE = {1, 63, 64, 65, 255, 256, 257, 513}


def run_tonemap(tracer, rgb, fields, in_place, what):
    height, width = rgb.shape[:2]
    p = tonemap_ref.params(**fields)
    arena = Arena(device_of(tracer), width, 1)
    d_in = arena.inout("d_rgb_in (in place)", rgb, 3) if in_place else arena.input("d_rgb_in", rgb, 3)
    d_state = arena.inout("d_state", np.zeros(8, dtype=np.uint32), 1)
    d_out = d_in if in_place else arena.output("d_rgb_out", width * height, 3)
    d_rgba = arena.output("d_rgba8_out", width * height, 1)
    tracer.tonemap_device(width, height, d_in.ptr, d_state.ptr, p, d_out.ptr, d_rgba.ptr, stream=stream())
    arena.check()
    want_rgb, want_rgba, want_state = tonemap_ref.frame(rgb, p)
    d_state.assert_is(want_state, what, every_word_written=False)
    d_out.assert_is(want_rgb, what, every_word_written=not in_place), d_rgba.assert_is(want_rgba, what)
    return want_state


@pytest.mark.parametrize("axis", list(LINEAR_SIZES))
@pytest.mark.parametrize("name", list(TONEMAP_PARAMS))
def test_tone_mapping(tracer, name, axis):
    for width, height in LINEAR_SIZES[axis]:
        rgb = tonemap_ref.noise(height, width, seed=3 * width + height)
        state = run_tonemap(tracer, rgb, TONEMAP_PARAMS[name], False, f"{width}x{height}, {name}")
        if name.startswith("metered"):
            assert tonemap_ref.info_of(state)["counted"] == width * height
        if width * height in IN_PLACE:
            run_tonemap(tracer, rgb, TONEMAP_PARAMS[name], True, f"{width}x{height}, {name}, in place")


# ---- bloom --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", list(BLOOM_SIZES))
def test_bloom(tracer, axis):
    """bloom_down's 16-texel tile and its staged border at levels 0 and 1; the bands are device_bloom's own."""
    from tests.test_gpu_bloom import assert_is_the_restatement

    for width, height in BLOOM_SIZES[axis]:
        rgb = bloom_ref.noise(height, width, seed=100 * width + height)
        assert_is_the_restatement(tracer, rgb, bloom_ref.params(levels=8), f"edges {width}x{height}")
