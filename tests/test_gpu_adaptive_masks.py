"""The adaptive builds of the render kernels under CONSTRUCTED stop masks, at all five tile shapes, tolerance 0.

tests/test_gpu_adaptive.py meets only the stop maps the rule itself produces: solid regions, so most tiles are all-stopped or all-active,
at tiles of 64 pixels (and 16 on `basic`).  Here the test sets the stopped bits itself: rt_hip_adaptive_pass_device leaves its 9-word block
with the caller between passes, so after pass 0 (nobody can stop: min_samples is two passes) a mask of tests/adaptive_masks.py is ORed
into the state words, every pass_sum word is overwritten with a NaN pattern, and pass 1 runs.  A stopped pixel must come back untouched,
word for word, and still show the oracle's pixel at S samples; an active one must have been traced, hold 2 S samples and show the oracle's
pixel at 2 S; every decision — beside hand-stopped neighbours — must be the serial restatement's; the work reported must be the active
pixels'.  The tile shape of every case is asked of the CPU plan dump, so that a change of tile policy cannot silently drop a shape.

Then the update kernel alone at frame sizes with 1-pixel sides and sides one past its 16 x 16 workgroup, and noise placed on the four
sides of a workgroup corner, where the 3 x 3 rule reads words another workgroup owns."""
import functools

import numpy as np
import pytest

from oracle import binding as oracle
from tests import adaptive_masks as masks
from tests import adaptive_plan
from tests import adaptive_reference as ref
from tests.test_gpu_progressive import BVH, H, SCENES, SEED, SM, W, reference

pytestmark = pytest.mark.gpu

STOPPED, COUNT = ref.STOPPED, ref.COUNT
PATTERN = np.uint32(0x7FC0BEEF)
SHAPE_OF = {16: 6, 32: 5, 48: 4, 80: 3, 192: 2}  # pass size -> pixels_log2 of a 37 x 23 frame (asserted through the plan dump)
OTHER_BUILDS = ["basic_tilted", "field50", "field300_bvh", "field1500", "dielectric_sm"]


def scene(name, spp, width, height):
    make = SCENES[name][0]
    return make(spp) if (width, height) == (W, H) else make(spp, width, height)


@functools.lru_cache(maxsize=None)
def oracle_frame(name, spp, width=W, height=H):
    """(rgba, rgb, segments) of the oracle at `spp` samples per pixel: computed once, shared, read-only."""
    if (width, height) == (W, H):
        return reference(name, spp)
    rgba, rgb, stats = oracle.render(scene(name, spp, width, height), width, height, seed=SEED, sm_materials=bool(SCENES[name][1] & SM))
    rgba.setflags(write=False), rgb.setflags(write=False)
    return rgba, rgb, stats["segments"]


def plan_of(name, size, width=W, height=H):
    """The launch plan of pass 1 — samples [size, 2 size) — from the CPU dump."""
    assert adaptive_plan.executable() is not None, "the plan dump program needs g++: without it nothing says which tile shape a pass takes"
    _, flags, _, build = SCENES[name]
    pod = scene(name, 2 * size, width, height)
    camera = 0 if build == (0, 0, 0) else 2
    (plan,) = adaptive_plan.plans([(pod.n_spheres, pod.n_planes, 1, width, height, 2 * size, camera, flags & (BVH | SM), size, size)])
    assert plan["adaptive"] == 1 and plan["chunks"] == size // 16, plan
    assert (plan["scan"], plan["planes"], plan["general_camera"]) == build, plan
    return plan


class Block:
    """The caller's 9 words per pixel on the host, as uint32: accum | state | pass_sum | moments."""

    def __init__(self, words, width, height):
        pixels = width * height
        words = words.view(np.uint32)
        self.accum = words[: 3 * pixels].reshape(height, width, 3).copy()
        self.state = words[3 * pixels : 4 * pixels].reshape(height, width).copy()
        self.pass_sum = words[4 * pixels : 7 * pixels].reshape(height, width, 3).copy()
        self.moments = words[7 * pixels :].reshape(height, width, 2).copy()

    def words(self):
        return np.concatenate([self.accum.ravel(), self.state.ravel(), self.pass_sum.ravel(), self.moments.ravel()])


def two_passes(tracer, name, size, mask, width, height):
    """The experiment: pass 0, the mask ORed into the state words and the pattern written over pass_sum by hand, pass 1.
    -> (the block before pass 1, the block after it, packed frame, float mean — both as uint32 —, the active count, the stats)"""
    import torch

    flags = SCENES[name][1]
    pixels = width * height
    want_first = oracle_frame(name, size, width, height)
    tracer.upload(scene(name, 2 * size, width, height))
    stream = torch.cuda.current_stream().cuda_stream
    block = torch.full((9 * pixels,), float("nan"), dtype=torch.float32, device="cuda:0")  # (pass 0 must read none of it)
    frame = torch.zeros((height, width), dtype=torch.int32, device="cuda:0")
    mean = torch.zeros((height, width, 3), dtype=torch.float32, device="cuda:0")
    active = torch.full((1,), -1, dtype=torch.int32, device="cuda:0")
    p = ref.params(min_samples=2 * size)

    def run(first):
        tracer.adaptive_pass_device(width, height, first, size, block.data_ptr(), frame.data_ptr(), seed=SEED, flags=flags, params=p, d_rgb_f32=mean.data_ptr(), d_active_pixels=active.data_ptr(), stream=stream)
        torch.cuda.synchronize()

    # pass 0: nobody can stop, and the state words hold `size`
    run(0)
    before = Block(block.cpu().numpy(), width, height)
    assert (before.state == size).all() and int(active.cpu().numpy()[0]) == pixels and tracer.stats()["primary_samples"] == pixels * size
    assert np.array_equal(frame.cpu().numpy().view(np.uint32), want_first[0]) and np.array_equal(mean.cpu().numpy().view(np.uint32), want_first[1].view(np.uint32))
    # the mask, by hand; all of pass_sum becomes the pattern a traced pixel must overwrite and a stopped one must keep
    before.state[mask] |= STOPPED
    before.pass_sum[:] = PATTERN
    block.copy_(torch.from_numpy(before.words().view(np.float32)))
    assert np.array_equal(block.cpu().numpy().view(np.uint32), before.words())  # (the copy kept the NaN payloads)

    run(size)
    return before, Block(block.cpu().numpy(), width, height), frame.cpu().numpy().view(np.uint32), mean.cpu().numpy().view(np.uint32), int(active.cpu().numpy()[0]), tracer.stats()


def two_passes_under_a_mask(tracer, name, size, family, width=W, height=H):
    """The experiment under one family's mask, and every assertion on it."""
    kernel = SCENES[name][2]
    plan = plan_of(name, size, width, height)
    if (width, height) == (W, H):
        assert plan["pixels_log2"] == SHAPE_OF[size], plan
    mask = masks.mask(family, width, height, plan["tile_w_log2"], plan["pixels_log2"])
    pixels = width * height
    p = ref.params(min_samples=2 * size)
    want_first, want_second = oracle_frame(name, size, width, height), oracle_frame(name, 2 * size, width, height)
    before, after, got_rgba, got_rgb, got_active, stats = two_passes(tracer, name, size, mask, width, height)
    where = f"{name}, passes of {size}, {family}, tiles of {1 << plan['tile_w_log2']} x {(1 << plan['pixels_log2']) >> plan['tile_w_log2']}"
    print(where, "-", int((~mask).sum()), "of", pixels, "pixels active;", {k: stats[k] for k in ("kernel", "primary_samples", "segments")}, "active after:", got_active)

    def differing(a, b, at):
        wrong = (a != b).reshape(height, width, -1).any(axis=-1) & at
        return f"{where}: {wrong.sum()} of {at.sum()} pixels, the first at (x, y) = {tuple(int(v) for v in np.argwhere(wrong)[0][::-1]) if wrong.any() else None}"

    # stopped pixels: neither read nor written, and finished at their own count
    assert np.array_equal(after.accum[mask], before.accum[mask]), "a stopped pixel's accum changed — " + differing(after.accum, before.accum, mask)
    assert np.array_equal(after.state[mask], before.state[mask]), "a stopped pixel's state changed — " + differing(after.state, before.state, mask)
    assert np.array_equal(after.moments[mask], before.moments[mask]), "a stopped pixel's moments changed — " + differing(after.moments, before.moments, mask)
    assert (after.pass_sum[mask] == PATTERN).all(), "a stopped pixel's pass_sum was written — " + differing(after.pass_sum, before.pass_sum, mask)
    assert np.array_equal(got_rgba[mask], want_first[0][mask]), "stopped pixels are not the oracle's at S — " + differing(got_rgba, want_first[0], mask)
    assert np.array_equal(got_rgb[mask], want_first[1].view(np.uint32)[mask]), "stopped pixels' means are not the oracle's at S — " + differing(got_rgb, want_first[1].view(np.uint32), mask)
    # active pixels: traced, 2 S samples, the oracle's pixel at 2 S
    live = ~mask
    assert (after.pass_sum[live] != PATTERN).all(), "an active pixel's pass_sum was not written — " + differing(after.pass_sum == PATTERN, np.zeros_like(after.pass_sum, dtype=bool), live)
    assert ((after.state[live] & COUNT) == 2 * size).all(), where
    assert np.array_equal(got_rgba[live], want_second[0][live]), "active pixels are not the oracle's at 2 S — " + differing(got_rgba, want_second[0], live)
    assert np.array_equal(got_rgb[live], want_second[1].view(np.uint32)[live]), "active pixels' means are not the oracle's at 2 S — " + differing(got_rgb, want_second[1].view(np.uint32), live)
    if size == 16:  # one chunk: the running sum went on by exactly the pass's fold
        with np.errstate(all="ignore"):
            assert np.array_equal(after.accum[live], (before.accum.view(np.float32)[live] + after.pass_sum.view(np.float32)[live]).view(np.uint32)), where
    # the decisions: min_samples = 2 S, so pass 1 really judges, and a hand-stopped neighbour counts as converged
    want_moments, want_state, want_rgba, want_rgb, want_active = ref.step(after.accum.view(np.float32), after.pass_sum.view(np.float32), before.moments.view(np.float32), before.state, size, False, True, p)
    assert np.array_equal(after.moments, want_moments.view(np.uint32)), differing(after.moments, want_moments.view(np.uint32), live | mask)
    assert np.array_equal(after.state, want_state), differing(after.state, want_state, live | mask)
    assert np.array_equal(got_rgba, want_rgba) and np.array_equal(got_rgb, want_rgb.view(np.uint32)), where
    assert got_active == want_active == int(((after.state & STOPPED) == 0).sum()), (where, got_active, want_active)
    # the work
    assert stats["kernel"] == kernel, (where, stats)
    assert stats["primary_samples"] == int(live.sum()) * size, (where, stats["primary_samples"], int(live.sum()) * size)
    if family == "all_stopped":
        assert stats["segments"] == 0 and got_active == 0, (where, stats, got_active)
        assert np.array_equal(after.words(), before.words()), where
    if family == "none_stopped":  # samples have streams of their own, so the difference of the oracle's counts is the pass's
        assert stats["segments"] == want_second[2] - want_first[2], (where, stats["segments"], want_second[2] - want_first[2])
    # ... and pixels have streams of their own, so the same experiment under the COMPLEMENT of the mask traces exactly the rest: a
    # stopped pixel's chunk that was traced anyway and then dropped by the fold changes no word of the block, and shows here
    complement = two_passes(tracer, name, size, ~mask, width, height)[5]
    assert stats["segments"] + complement["segments"] == want_second[2] - want_first[2], (where, stats["segments"], complement["segments"], want_second[2] - want_first[2])
    return mask, plan


@pytest.mark.parametrize("family", masks.FAMILIES)
@pytest.mark.parametrize("size", sorted(SHAPE_OF))
def test_basic_at_every_tile_shape_under_every_mask(tracer, size, family):
    two_passes_under_a_mask(tracer, "basic", size, family)


@pytest.mark.parametrize("family", ["random_half", "one_active_per_tile", "ragged_edge_only", "all_stopped"])
@pytest.mark.parametrize("size", [32, 80])
@pytest.mark.parametrize("name", OTHER_BUILDS)
def test_the_other_adaptive_builds_at_a_per_pixel_and_a_channel_per_lane_shape(tracer, name, size, family):
    _, plan = two_passes_under_a_mask(tracer, name, size, family)
    assert (3 << plan["pixels_log2"] <= 64) == (size == 80)


@pytest.mark.parametrize("width,height", [(64, 16), (128, 32)])
def test_the_single_active_pixel_walks_the_mask_in_whole_tiles_of_64(tracer, width, height):
    """No ragged edge: 16 and 64 tiles of 8 x 8; at 128 x 32 every one of the 64 bit positions is the single active pixel of some tile."""
    mask, plan = two_passes_under_a_mask(tracer, "basic", 16, "one_active_per_tile", width, height)
    assert (plan["pixels_log2"], plan["tile_w_log2"]) == (6, 3)
    g = masks.Geometry(width, height, 3, 6)
    assert (~mask).sum() == g.tiles_x * g.tiles_y == width * height // 64
    assert len(set(g.index[~mask].tolist())) == min(64, g.tiles_x * g.tiles_y)


# ---- the update kernel alone ------------------------------------------------------------------------------------------------------------
def two_update_passes(tracer, width, height, noisy, seed):
    """Two passes of 16 through rt_hip_adaptive_update_device alone, each against the restatement.  `noisy`: bool[height, width] — those
    pixels' pass sums are 0.1 n then 1.9 n times their level, the others' agree (they converge at pass 2 under the defaults: two equal
    luminances have variance 0; the noisy ones' standard error is 0.9 of their mean against a limit of 0.03).  -> the state words."""
    import torch

    rng = np.random.default_rng(seed)
    level = rng.uniform(0.1, 1.0, size=(height, width, 3))
    accum = np.zeros((height, width, 3), dtype=np.float32)
    moments = np.full((height, width, 2), np.nan, dtype=np.float32)
    state = np.full((height, width), 0xFFFFFFFF, dtype=np.uint32)  # (the first pass writes them and does not read them)
    stream = torch.cuda.current_stream().cuda_stream
    p = ref.params()
    for k, factor in enumerate((0.1, 1.9)):
        pass_sum = (np.where(noisy[..., None], factor, 1.0) * level * 16).astype(np.float32)
        accum = (pass_sum if k == 0 else accum + pass_sum).astype(np.float32)
        d_accum, d_pass_sum = torch.from_numpy(accum).to("cuda:0"), torch.from_numpy(pass_sum).to("cuda:0")
        d_moments, d_state = torch.from_numpy(moments.copy()).to("cuda:0"), torch.from_numpy(state.view(np.int32).copy()).to("cuda:0")
        d_rgba, d_rgb = torch.zeros((height, width), dtype=torch.int32, device="cuda:0"), torch.zeros((height, width, 3), dtype=torch.float32, device="cuda:0")
        d_active = torch.full((1,), -1, dtype=torch.int32, device="cuda:0")
        tracer.adaptive_update_device(width, height, 16, k == 0, True, d_accum.data_ptr(), d_pass_sum.data_ptr(), d_moments.data_ptr(), d_state.data_ptr(), d_rgba.data_ptr(), params=p, d_rgb_out=d_rgb.data_ptr(),
                                      d_active_pixels=d_active.data_ptr(), stream=stream)
        torch.cuda.synchronize()
        want_moments, want_state, want_rgba, want_rgb, want_active = ref.step(accum, pass_sum, moments, state, 16, k == 0, True, p)
        got_state = d_state.cpu().numpy().view(np.uint32)
        assert np.array_equal(got_state, want_state), (k, np.argwhere(got_state != want_state)[:8].tolist())
        assert np.array_equal(d_moments.cpu().numpy().view(np.uint32), want_moments.view(np.uint32)), k
        assert np.array_equal(d_rgba.cpu().numpy().view(np.uint32), want_rgba) and np.array_equal(d_rgb.cpu().numpy().view(np.uint32), want_rgb.view(np.uint32)), k
        assert int(d_active.cpu().numpy()[0]) == want_active == int(((got_state & STOPPED) == 0).sum())
        moments, state = want_moments, got_state
        assert ((state & COUNT) == 16 * (k + 1)).all()
    return state


def dilated(noisy):
    """The 3 x 3 dilation of a set of pixels, clipped to the frame — by hand, without the restatement."""
    height, width = noisy.shape
    out = np.zeros_like(noisy)
    for y, x in np.argwhere(noisy):
        out[max(y - 1, 0) : min(y + 2, height), max(x - 1, 0) : min(x + 2, width)] = True
    return out


@pytest.mark.parametrize("layout", ["sparse_noise", "all_flat", "all_noisy"])
@pytest.mark.parametrize("width,height", [(1, 1), (1, 40), (40, 1), (17, 17), (16, 33), (33, 16)])
def test_the_update_kernel_at_sides_of_one_pixel_and_one_past_a_workgroup(tracer, width, height, layout):
    y, x = np.mgrid[0:height, 0:width]
    noisy = {"sparse_noise": (3 * x + 5 * y) % 11 == 0, "all_flat": np.zeros((height, width), dtype=bool), "all_noisy": np.ones((height, width), dtype=bool)}[layout]
    assert noisy[0, 0] == (layout != "all_flat")  # (the 1 x 1 frame is noisy under sparse_noise, flat under all_flat)
    state = two_update_passes(tracer, width, height, noisy, seed=width * 64 + height)
    assert np.array_equal((state & STOPPED) == 0, dilated(noisy)), np.argwhere(((state & STOPPED) == 0) != dilated(noisy))[:8].tolist()
    if layout == "sparse_noise" and width * height > 1:
        assert ((state & STOPPED) != 0).any() and ((state & STOPPED) == 0).any()


CORNER = [(15, 15), (16, 15), (15, 16), (16, 16)]  # (x, y): the four sides of the corner four 16 x 16 workgroups share


@pytest.mark.parametrize("which", [[0], [1], [2], [3], [0, 1, 2, 3]])
def test_noise_on_the_four_sides_of_a_workgroup_corner_keeps_exactly_its_neighbourhood_going(tracer, which):
    """33 x 33: the halo lanes read words another workgroup owns.  The pixels not stopped after pass 2 are the 3 x 3 dilation of the
    noisy set — asserted by hand, besides the equality with the restatement."""
    noisy = np.zeros((33, 33), dtype=bool)
    for x, y in (CORNER[i] for i in which):
        noisy[y, x] = True
    state = two_update_passes(tracer, 33, 33, noisy, seed=33 + sum(which))
    going = (state & STOPPED) == 0
    want = np.zeros((33, 33), dtype=bool)
    for x, y in (CORNER[i] for i in which):
        want[y - 1 : y + 2, x - 1 : x + 2] = True
    assert want.sum() == (9 if len(which) == 1 else 16)
    assert np.array_equal(going, want), np.argwhere(going != want)[:8].tolist()
