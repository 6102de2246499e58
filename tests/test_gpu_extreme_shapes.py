"""Frames at the extremes of shape through every kernel that takes a frame, tolerance 0 throughout.

The suite's largest frame was 3840 x 2160 and none was far from 16:9.  Here: frames one and three pixels wide and up to 131070 rows high,
frames one and three rows high and up to 262145 pixels wide, one row past the last whole tile at 70000 rows, a frame smaller than one
tile, and the post-process entry points at the 32768 pixels a side they accept.  Where it can go wrong is arithmetic no other test
reaches: a tile's place from `(gridDim.y - 1 - blockIdx.y) * tile_h` and four tiles side by side per workgroup, the rolling kernels'
item -> pixel -> (row, column) division, a grid whose y dimension is the frame's, the tail lanes of a run of four.

tests/extreme_shapes.py holds the case table, the references (each computed once) and the kernel and tile shape every frame is planned
with; tests/test_plan_frame_extremes.py holds that table to the plan on the CPU, and that every accepted frame's grid is in range — no
test here launches a grid that is not.  A device frame is rendered into the middle of a longer buffer filled with a sentinel in front
and behind, so a tile placed a row off shows even where it lands outside the frame.  RT_HIP_FLAG_FAST stays out: its per-pixel bound
has a table of its own (tests/fast_cases.py)."""
import re

import numpy as np
import pytest

import rt_amd
from rt_amd import capi
from tests import adaptive_masks as masks
from tests import adaptive_plan
from tests import adaptive_reference as adaptive_ref
from tests import denoise_reference as guide_ref
from tests import extreme_shapes as es
from tests import partition_cases as pc
from tests import reproject_reference as reproject_ref
from tests import temporal_cases
from tests import tonemap_reference as tonemap_ref
from tests import upsample_reference as upsample_ref
from tests.test_gpu_denoise import assert_filter_is_the_restatement, device_guide
from tests.test_gpu_temporal import device_step
from tests.test_gpu_tonemap import assert_is_the_restatement as assert_tonemap_is_the_restatement
from tests.test_gpu_upsample import assert_is_the_restatement as assert_upsample_is_the_restatement
from tests.test_sky_band_rule import gpu_scene

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A  # alpha byte 0x5A: no finished pixel (every one has alpha 0xFF)
SEED = es.SEED
TALL, WIDE = es.TALL, es.WIDE
CAP = 32768  # max_frame_side of the post-process and adaptive entry points
INVALID_ARGUMENT = 1


@pytest.fixture(autouse=True)
def _no_table_outlives_a_test(tracer):
    yield
    tracer.set_emission(None)  # (the session's context is shared: no other test file sees a table)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_frame(got_rgba, got_rgb, want_rgba, want_rgb, what):
    """every packed pixel and every word of the float mean; the message says how much differs and where first"""
    bad = (bits(got_rgb) != bits(want_rgb)).any(axis=-1)
    if bad.any():
        y, x = np.argwhere(bad)[0]
        raise AssertionError(f"{what}: the float mean differs in {int(bad.sum())} of {bad.size} pixels ({int(bad.any(axis=1).sum())} rows); first at (x, y) = ({x}, {y}): gpu {got_rgb[y, x]} against {want_rgb[y, x]}")
    bad = got_rgba != want_rgba
    if bad.any():
        y, x = np.argwhere(bad)[0]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} packed pixels differ; first at (x, y) = ({x}, {y}): gpu {got_rgba[y, x]:08x} against {want_rgba[y, x]:08x}")


def pad_rows(width):
    """rows of sentinel in front of and behind a device frame: at least two, and at least 64 words"""
    return 2 + 64 // width


def render_into_sentinels(tracer, size, flags=0, partition=None, rows=None):
    """rt_hip_render_device of the resident scene into the middle of sentinel-filled buffers: (rgba, float mean, stats) of the `rows`
    rows the launch owns (the whole frame's by default), after asserting that not one word in front of or behind them was written"""
    import torch

    width, height = size
    rows = height if rows is None else rows
    pad = pad_rows(width)
    frame = torch.full((rows + 2 * pad, width), SENTINEL, dtype=torch.int32, device="cuda:0")
    mean = torch.full((rows + 2 * pad, width, 3), float("nan"), dtype=torch.float32, device="cuda:0")
    tracer.render_device(width, height, frame.data_ptr() + 4 * pad * width, seed=SEED, flags=flags, partition=partition, d_rgb_f32=mean.data_ptr() + 12 * pad * width, stream=torch.cuda.current_stream().cuda_stream)
    stats = tracer.stats()
    torch.cuda.synchronize()
    rgba, rgb = frame.cpu().numpy().view(np.uint32), mean.cpu().numpy()
    for name, outside in (("in front of", np.s_[:pad]), ("behind", np.s_[pad + rows :])):
        touched = rgba[outside] != SENTINEL
        assert not touched.any(), f"{int(touched.sum())} packed words {name} the frame's {rows} rows were written; first {np.argwhere(touched)[0]} (row, x) into that margin"
        touched = ~np.isnan(rgb[outside])
        assert not touched.any(), f"{int(touched.sum())} floats of the mean {name} the frame's {rows} rows were written; first {np.argwhere(touched)[0]} into that margin"
    return rgba[pad : pad + rows], rgb[pad : pad + rows], stats


# ---- a. one-shot frames ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,spp,size", es.ONE_SHOT, ids=[es.case_id(*case) for case in es.ONE_SHOT])
def test_a_one_shot_frame_into_a_host_frame_and_into_hbm(tracer, name, spp, size):
    build, pod = es.BUILDS[name], es.pod_of(name, spp)
    want_rgba, want_rgb, want_stats = es.reference(name, spp, size)
    width, height = size
    tracer.set_emission(build.table)
    for host in (1, 0):
        kernel = es.EXPECTED[(name, spp, size)][1 - host][0]
        assert es.tile_of(es.plan(name, spp, size, host)) == es.EXPECTED[(name, spp, size)][1 - host]  # (the table is the plan's: a change of policy cannot silently empty a case)
        what = f"{es.case_id(name, spp, size)} into {'a page-locked host frame (rt_hip_render)' if host else 'HBM (rt_hip_render_device)'}, planned as {es.EXPECTED[(name, spp, size)][1 - host]}"
        if host:
            out = np.full((height, width), SENTINEL, dtype=np.uint32)
            rgba, rgb, stats = tracer.render(pod, width, height, seed=SEED, flags=build.flags, want_rgb=True, out=out)
        else:
            tracer.upload(pod)
            rgba, rgb, stats = render_into_sentinels(tracer, size, build.flags)
        assert_frame(rgba, rgb, want_rgba, want_rgb, what)
        assert stats["kernel"] == kernel, (what, stats)
        assert stats["primary_samples"] == want_stats["primary_samples"] == width * height * spp and stats["segments"] == want_stats["segments"], (what, stats, want_stats)


# ---- b. the sky band ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,band", [((5, CAP), True), ((5, CAP + 1), False), ((65537, 3), False)], ids=["5x32768-at-the-cap", "5x32769-past-the-cap", "65537x3-no-strip"])
def test_the_sky_band_at_its_cap_and_past_it(monkeypatch, capfd, size, band):
    """A frame of 32768 rows is the tallest the band's rule takes: the band runs, over the rows the rule gives on the CPU, and the scene's
    kernel is launched over the rest; one row more, or three rows in all, and every row is the scene kernel's.  The band's own log line (a
    context created under RT_HIP_SKY_BAND_LOG=1) says which — two frames that both took no band would prove nothing."""
    width, height = size
    spp = 17
    pod = gpu_scene("basic").set_sampling(samples_per_pixel=spp).describe(*es.CAMERA_SIZE)
    want_rows = es.band_rows(pod, size)
    assert (want_rows > 0) == band and want_rows < height, (size, want_rows)
    want_rgba, want_rgb, want_stats = es.oracle.render(pod, width, height, seed=SEED)
    monkeypatch.setenv("RT_HIP_SKY_BAND_LOG", "1")
    monkeypatch.delenv("RT_HIP_SKY_BAND", raising=False)
    with rt_amd.HipRayTracer(device=0) as tracer:
        for host in (1, 0):
            capfd.readouterr()
            if host:
                rgba, rgb, stats = tracer.render(pod, width, height, seed=SEED, want_rgb=True)
            else:
                tracer.upload(pod)
                rgba, rgb, stats = render_into_sentinels(tracer, size)
            logged = [int(found.group(1)) for found in re.finditer(r"rt_hip sky band: rows (\d+) of \d+", capfd.readouterr().err)]
            what = f"{width} x {height}, {'host frame' if host else 'HBM'}"
            assert logged == [want_rows], (what, logged, want_rows)
            assert_frame(rgba, rgb, want_rgba, want_rgb, what)
            assert stats["kernel"] == "small" and stats["primary_samples"] == width * height * spp and stats["segments"] == want_stats["segments"], (what, stats, want_stats)


# ---- c. the preview ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [TALL, WIDE], ids=["3x70001", "70001x1"])
def test_the_preview(tracer, size):
    pod = es.pod_of("preview", 1)
    want_rgba, want_rgb, want_stats = es.reference("preview", 1, size)
    width, height = size
    rgba, rgb, stats = tracer.render(pod, width, height, seed=SEED, flags=capi.RT_HIP_FLAG_PREVIEW, want_rgb=True)
    assert_frame(rgba, rgb, want_rgba, want_rgb, f"preview {width} x {height}, host frame")
    assert stats["kernel"] == "preview" and stats["segments"] == width * height, stats
    tracer.upload(pod)
    rgba, rgb, stats = render_into_sentinels(tracer, size, capi.RT_HIP_FLAG_PREVIEW)
    assert_frame(rgba, rgb, want_rgba, want_rgb, f"preview {width} x {height}, HBM")
    assert stats["kernel"] == "preview" and stats["segments"] == width * height, stats


# ---- d. ranks and assembly -----------------------------------------------------------------------------------------------------------------------
def row_table(height, world, stripe):
    """(rank, local row) of every image row as two arrays, and the rows per rank: tests/partition_cases.row_table's plain loops"""
    table, counts = pc.row_table(height, world, stripe)
    table = np.array(table, dtype=np.int64)
    return table[:, 0], table[:, 1], counts


def test_three_ranks_of_a_tall_frame_and_their_assembly(tracer):
    """3 x 70001 as ranks 0..2 of 3 under stripes of 8 rows: every rank's rows are the whole frame's, nothing is written past them, and
    rt_hip_assemble_device at height 70001 — the launch whose grid had one workgroup row per image row — puts the frame together."""
    import torch

    name, spp, size, world, stripe = "small_auto", 64, TALL, 3, 8
    width, height = size
    want_rgba, want_rgb, want_stats = es.reference(name, spp, size)
    rank_of, local_of, counts = row_table(height, world, stripe)
    padded = rt_amd.padded_local_rows(height, world, stripe)
    assert padded == max(counts) and sum(counts) == height
    tracer.upload(es.pod_of(name, spp))
    gathered = np.full((world, padded, width), 0xEE000000, dtype=np.uint32)
    segments = 0
    for rank in range(world):
        p = es.plan(name, spp, size, 0, rows=counts[rank])
        rgba, rgb, stats = render_into_sentinels(tracer, size, partition=(rank, world, stripe), rows=counts[rank])
        rows = np.flatnonzero(rank_of == rank)
        assert np.array_equal(local_of[rows], np.arange(counts[rank]))
        assert_frame(rgba, rgb, want_rgba[rows], want_rgb[rows], f"rank {rank} of {world}, stripes of {stripe} rows, {counts[rank]} rows")
        assert stats["kernel_variant"] == p["variant"] and stats["primary_samples"] == counts[rank] * width * spp, (rank, stats, p)
        segments += stats["segments"]
        gathered[rank, : counts[rank]] = rgba
    assert segments == want_stats["segments"]
    d_gathered = torch.from_numpy(gathered.view(np.int32)).to("cuda:0")
    for host in (False, True):
        frame = torch.full((height + 2, width), SENTINEL, dtype=torch.int32, **({"pin_memory": True} if host else {"device": "cuda:0"}))
        tracer.assemble_device(width, height, world, stripe, d_gathered.data_ptr(), frame.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got = frame.cpu().numpy().view(np.uint32)
        bad = got[:height] != want_rgba
        assert not bad.any(), f"assembled into {'a page-locked host' if host else 'an HBM'} frame: {int(bad.sum())} of {bad.size} pixels differ; first at (y, x) = {tuple(np.argwhere(bad)[0])}"
        assert (got[height:] == SENTINEL).all()


def test_assemble_alone_at_131070_rows(tracer):
    """rt_hip_assemble_device on words that say where they came from: 2 x 131070, four ranks, stripes of 5 rows — twice the rows a grid
    holds in y, so every workgroup takes two — against numpy indexing through the row table; poisoned padding rows, a sentinel behind."""
    import torch

    width, height, world, stripe = 2, 131070, 4, 5
    rank_of, local_of, counts = row_table(height, world, stripe)
    padded = rt_amd.padded_local_rows(height, world, stripe)
    assert padded == max(counts)
    x = np.arange(width, dtype=np.uint32)
    gathered = np.full((world, padded, width), 0xEE000000, dtype=np.uint32) | x
    for rank in range(world):
        gathered[rank, : counts[rank]] = (np.uint32(rank) << 28) | (np.arange(counts[rank], dtype=np.uint32)[:, None] << 4) | x
    want = gathered[rank_of, local_of]
    assert len(np.unique(want)) == want.size and not ((want & 0xFF000000) == 0xEE000000).any()
    d_gathered = torch.from_numpy(gathered.view(np.int32)).to("cuda:0")
    for host in (False, True):
        frame = torch.full((height + 2, width), SENTINEL, dtype=torch.int32, **({"pin_memory": True} if host else {"device": "cuda:0"}))
        tracer.assemble_device(width, height, world, stripe, d_gathered.data_ptr(), frame.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got = frame.cpu().numpy().view(np.uint32)
        bad = got[:height] != want
        assert not bad.any(), (f"{'host' if host else 'HBM'} frame: {int(bad.sum())} of {bad.size} words differ; first at (y, x) = {tuple(np.argwhere(bad)[0])}: {got[:height][bad][0]:08x} against {want[bad][0]:08x} "
                               "= (rank << 28 | local row << 4 | x)")
        assert (got[height:] == SENTINEL).all(), "words beyond the frame were written"


# ---- e. passes -----------------------------------------------------------------------------------------------------------------------------------
def abandon_what_is_in_flight(tracer):
    """the session's context keeps its accumulations from test to test: a pass of a frame no test renders leaves keys that differ from every test's"""
    tracer.render_progressive(es.pod_of("small_auto", 16), 8, 8, seed=SEED + 1000, pass_samples=16)
    tracer.render_adaptive(es.pod_of("small_auto", 16), 8, 8, seed=SEED + 1000, pass_samples=16)


def test_a_progressive_frame_in_passes_of_16(tracer):
    """3 x 70001 at 40 samples: passes of 16, 16 and 8; after every pass the frame is the one-shot frame at the samples done"""
    width, height = TALL
    pod = es.pod_of("small_auto", 40)
    abandon_what_is_in_flight(tracer)
    for done in (16, 32, 40):
        rgba, rgb, stats, progress = tracer.render_progressive(pod, width, height, seed=SEED, pass_samples=16, want_rgb=True)
        assert progress["samples_done"] == done and progress["samples_total"] == 40, progress
        want_rgba, want_rgb, _ = es.reference("small_auto", done, TALL)
        assert_frame(rgba, rgb, want_rgba, want_rgb, f"progressive 3 x 70001 after {done} samples")
        assert stats["kernel"] == "resident" and stats["primary_samples"] == width * height * (done - max(0, (done - 1) // 16 * 16)), stats


@pytest.mark.parametrize("size", [TALL, (CAP, 2)], ids=["3x70001", "32768x2"])
def test_adaptive_passes_with_min_samples_above_the_cap(tracer, size):
    """no pixel may stop before min_samples = 64 and the frame has 32: two whole passes, each the one-shot frame at its count.  (3 x 70001
    is refused by name — 70001 rows are more than the adaptive entry points take — and nothing is launched.)"""
    width, height = size
    pod = es.pod_of("small_auto", 32)
    abandon_what_is_in_flight(tracer)
    p = adaptive_ref.params(min_samples=64)
    if height > CAP:
        out = np.full((height, width), SENTINEL, dtype=np.uint32)
        with pytest.raises(rt_amd.RtHipError) as refused:
            tracer.render_adaptive(pod, width, height, seed=SEED, pass_samples=16, params=p, out=out)
        assert refused.value.status == INVALID_ARGUMENT and f"rt_hip_render_adaptive: frame {width}x{height}" in str(refused.value), str(refused.value)
        assert (out == SENTINEL).all()
        return
    for done in (16, 32):
        rgba, rgb, counts, stats, info = tracer.render_adaptive(pod, width, height, seed=SEED, pass_samples=16, params=p, want_rgb=True)
        assert (counts == done).all() and info["samples_done"] == done and info["complete"] == (1 if done == 32 else 0), info
        want_rgba, want_rgb, _ = es.reference("small_auto", done, size)
        assert_frame(rgba, rgb, want_rgba, want_rgb, f"adaptive {width} x {height} after {done} samples")
        assert stats["kernel"] == "resident" and stats["primary_samples"] == width * height * 16, stats


@pytest.mark.parametrize("size", [(3, CAP), (CAP, 2), (CAP, 24)], ids=["3x32768", "32768x2", "32768x24"])
def test_an_adaptive_pass_under_a_mask_that_stops_the_first_and_the_last_tile_row(tracer, size):
    """Two device-level passes of 16 samples; between them the pixels of the first and of the last tile row are stopped by hand (the
    tiles are the plan's: tests/adaptive_masks.Geometry).  A stopped pixel stays the one-shot frame's at 16 samples and no word of its
    block is touched; every other pixel is the frame's at 32.  At the cap of the adaptive entry points in each direction; 32768 x 2 is ONE
    row of tiles, first and last at once — every pixel is stopped and the pass traces nothing — and 32768 x 24 is three."""
    import torch

    width, height = size
    pixels = width * height
    pod = es.pod_of("small_auto", 32)
    (plan,) = adaptive_plan.plans([(pod.n_spheres, pod.n_planes, 1, width, height, 32, 0, 0, 16, 16)])
    assert plan["adaptive"] == 1 and plan["grid_y"] <= 65535, plan
    g = masks.Geometry(width, height, plan["tile_w_log2"], plan["pixels_log2"])
    mask = (g.tile_y == 0) | (g.tile_y == g.tiles_y - 1)
    assert 0 < mask.sum() < pixels or g.tiles_y <= 2
    first, second = es.reference("small_auto", 16, size), es.reference("small_auto", 32, size)
    tracer.upload(pod)
    stream = torch.cuda.current_stream().cuda_stream
    block = torch.full((9 * pixels,), float("nan"), dtype=torch.float32, device="cuda:0")
    frame = torch.zeros((height, width), dtype=torch.int32, device="cuda:0")
    mean = torch.zeros((height, width, 3), dtype=torch.float32, device="cuda:0")
    active = torch.full((1,), -1, dtype=torch.int32, device="cuda:0")
    p = adaptive_ref.params(min_samples=64)

    def run(first_sample):
        tracer.adaptive_pass_device(width, height, first_sample, 16, block.data_ptr(), frame.data_ptr(), seed=SEED, params=p, d_rgb_f32=mean.data_ptr(), d_active_pixels=active.data_ptr(), stream=stream)
        torch.cuda.synchronize()
        return frame.cpu().numpy().view(np.uint32), mean.cpu().numpy()

    rgba, rgb = run(0)
    assert_frame(rgba, rgb, first[0], first[1], f"adaptive pass 0, {width} x {height}")
    before = block.cpu().numpy().view(np.uint32).copy()
    state = before[3 * pixels : 4 * pixels].reshape(height, width)
    assert (state == 16).all() and int(active.cpu().numpy()[0]) == pixels
    state[mask] |= adaptive_ref.STOPPED
    block.copy_(torch.from_numpy(before.view(np.float32)))
    rgba, rgb = run(16)
    stats = tracer.stats()
    after = block.cpu().numpy().view(np.uint32)
    want_rgba, want_rgb = np.where(mask, first[0], second[0]), np.where(mask[..., None], first[1], second[1])
    assert_frame(rgba, rgb, want_rgba, want_rgb, f"adaptive pass 1 under the mask, {width} x {height}, tiles of {g.tile_w} x {g.tile_h}")
    assert stats["primary_samples"] == int((~mask).sum()) * 16, stats
    for name, words, per_pixel in (("accum", np.s_[: 3 * pixels], 3), ("state", np.s_[3 * pixels : 4 * pixels], 1), ("pass_sum", np.s_[4 * pixels : 7 * pixels], 3), ("moments", np.s_[7 * pixels :], 2)):
        changed = (after[words] != before[words]).reshape(height, width, per_pixel).any(axis=-1)
        assert not (changed & mask).any(), f"{name} of {int((changed & mask).sum())} stopped pixels changed"
    assert ((after[3 * pixels : 4 * pixels].reshape(height, width)[~mask] & adaptive_ref.COUNT) == 32).all()


# ---- f. the post-process entry points at their cap -----------------------------------------------------------------------------------------------
CAP_SHAPES = [(CAP, 1), (1, CAP), (3, CAP), (CAP, 3)]
BOXES = capi.RT_HIP_FLAG_TRACE_BOXES


def shape_id(size):
    return f"{size[0]}x{size[1]}"


@pytest.mark.parametrize("boxes", [False, True], ids=["spheres", "boxes"])
@pytest.mark.parametrize("size", CAP_SHAPES, ids=shape_id)
def test_the_guide_at_the_cap(tracer, size, boxes):
    pod = es.pod_of("boxes_resident" if boxes else "small_auto", 16)
    width, height = size
    got = device_guide(tracer, pod, width, height, BOXES if boxes else 0)
    want = guide_ref.compose_guide(pod, width, height, boxes=boxes)
    bad = (bits(got) != bits(want)).any(axis=-1)
    assert not bad.any(), f"{int(bad.sum())} of {bad.size} guide records differ; first at (y, x) = {tuple(np.argwhere(bad)[0])}"
    assert len(np.unique(bits(want)[..., 7])) > 1  # (not one surface: sky and scene)


@pytest.mark.parametrize("iterations", [1, 2, 5])
@pytest.mark.parametrize("size", CAP_SHAPES, ids=shape_id)
def test_the_filter_at_the_cap(tracer, size, iterations):
    """1, 2 and 5 iterations: all three builds of atrous_pass; at 5 the taps reach 16 pixels, past both sides of a frame 3 wide"""
    width, height = size
    pod = es.pod_of("small_auto", 4)
    image = es.reference("small_auto", 4, size)[1]
    guide = guide_ref.compose_guide(pod, width, height)
    assert_filter_is_the_restatement(tracer, image, guide, guide_ref.params(iterations=iterations), f"{width} x {height}, {iterations} iterations")


@pytest.mark.parametrize("size", CAP_SHAPES, ids=shape_id)
def test_a_reprojection_step_at_the_cap(tracer, size):
    """a dolly move: the history of the frame before, found again through both cameras"""
    width, height = size
    camera = temporal_cases.toml_scene("basic", *es.CAMERA_SIZE), temporal_cases.toml_scene("basic", *es.CAMERA_SIZE, position=(0.0, 1.0, 2.6))
    guides = [guide_ref.compose_guide(pod, width, height) for pod in camera]
    means = [es.oracle.render(pod, width, height, seed=SEED + i)[1] for i, pod in enumerate(camera)]
    prev_rgb, prev_record, _ = reproject_ref.frame(camera[0], guides[0], means[0], 16)
    want_rgb, want_record, want_found = reproject_ref.frame(camera[1], guides[1], means[1], 16, reproject_ref.matrix_of(camera[0]), prev_rgb, prev_record)
    got_rgb, got_record, got_found = device_step(tracer, camera[1], guides[1], means[1], 16, prev=(reproject_ref.matrix_of(camera[0]), prev_rgb, prev_record))
    assert 0 < want_found < width * height or width * height < 4, want_found
    assert np.array_equal(bits(got_rgb), bits(want_rgb)) and np.array_equal(bits(got_record), bits(want_record)) and got_found == want_found, (size, got_found, want_found)


@pytest.mark.parametrize("factor", [2, 3])
@pytest.mark.parametrize("size", CAP_SHAPES, ids=shape_id)
def test_an_upsampled_frame_at_the_cap(tracer, size, factor):
    width, height = size
    status, _, w, h = upsample_ref.low_size(width, height, factor)
    assert status == 0
    assert (w, h) == (-(-width // factor), -(-height // factor))
    pod = es.pod_of("small_auto", 4)
    low = es.oracle.render(pod, w, h, seed=SEED)[1]
    assert_upsample_is_the_restatement(tracer, low, guide_ref.compose_guide(pod, w, h), guide_ref.compose_guide(pod, width, height), upsample_ref.params(), f"{width} x {height} from {w} x {h}")


@pytest.mark.parametrize("size", CAP_SHAPES + [(CAP - 1, 1)], ids=shape_id)
def test_tone_mapping_at_the_cap(tracer, size):
    """all three curves; 32768 x 3 is 24576 runs of four pixels, 32767 x 1 ends in a tail of three"""
    width, height = size
    rgb = tonemap_ref.noise(height, width, seed=width + height)
    for curve in tonemap_ref.CURVES:
        assert_tonemap_is_the_restatement(tracer, rgb, tonemap_ref.params(curve=curve), f"{width}x{height} / curve {curve}")


def test_one_pixel_past_the_cap_is_refused_by_name_and_nothing_is_launched(tracer):
    """guide, filter, reprojection and tone mapping take 32768 pixels a side: 32769 is refused with the entry point's name and the frame's
    size before anything is enqueued.  (rt_hip_upsample_device's own limit is 2^22 a side: tests/test_gpu_upsample.py refuses one past it.)"""
    import torch

    tracer.upload(es.pod_of("small_auto", 4))
    side = CAP + 1
    words = torch.full((side * 8 * 2,), float("nan"), dtype=torch.float32, device="cuda:0")  # room for a guide of 32769 x 2: nothing may reach it
    rgb = torch.full((side * 3 * 2,), float("nan"), dtype=torch.float32, device="cuda:0")
    out = torch.full((side * 3 * 2,), float("nan"), dtype=torch.float32, device="cuda:0")
    record = torch.full((side * 8 * 2,), float("nan"), dtype=torch.float32, device="cuda:0")
    state = torch.zeros(8, dtype=torch.int32, device="cuda:0")
    for width, height in ((side, 1), (1, side)):
        calls = {
            "rt_hip_guide_device": lambda: tracer.guide_device(width, height, words.data_ptr()),
            "rt_hip_denoise_device": lambda: tracer.denoise_device(width, height, rgb.data_ptr(), words.data_ptr(), None, out.data_ptr(), None),
            "rt_hip_reproject_device": lambda: tracer.reproject_device(width, height, None, words.data_ptr(), rgb.data_ptr(), 16, None, None, None, out.data_ptr(), record.data_ptr()),
            "rt_hip_tonemap_device": lambda: tracer.tonemap_device(width, height, rgb.data_ptr(), state.data_ptr(), None, out.data_ptr(), None),
        }
        for entry, call in calls.items():
            with pytest.raises(rt_amd.RtHipError) as refused:
                call()
            assert refused.value.status == INVALID_ARGUMENT and f"{entry}: frame {width}x{height}" in str(refused.value), (entry, str(refused.value))
    torch.cuda.synchronize()
    assert bool(torch.isnan(words).all()) and bool(torch.isnan(out).all()) and bool(torch.isnan(record).all()) and not state.cpu().numpy().any()
