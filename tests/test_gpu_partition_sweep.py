"""Every build family of the render kernels launched on every stripe shape of tests/partition_cases.py, every rank of it, and held bit
for bit — packed pixels and float mean, tolerance 0 — to ONE whole-frame CPU reference per (build, sample count), whose rows
tests/partition_cases.row_table picks (tests/test_partition_rows.py ties every reference's own `partition` to that table on the CPU).

include/rt_hip.h promises that the assembled image does not depend on `world`, for every build; before this file only the
scalar-register kernel had met more than one shape.  Per rank the buffers are two rows longer than rt_hip_padded_local_rows says and
pre-filled with a sentinel (a packed word whose alpha byte is not 0xFF; NaN in the float mean and in a pass's accumulator):

* rows [0, local_rows) are the reference frame's rows of that rank; every row from local_rows on still holds the sentinel;
* primary_samples = local_rows x width x samples, the ranks' segments add up to the reference's, kernel_variant is the plan's
  (tests/lds_plan.py, tests/light_plan.py asked with the rank's rows);
* a rank without rows returns RT_HIP_OK, writes nothing, reports no samples and no segments, and the next render on the context is right.

Then assemble_stripes on its own (words that say where they came from, poisoned padding rows), direct-frame members of a multi-member
context (frame_rows != 0: a pixel goes to its IMAGE row) over the builds such a context takes, and a frame with a sky band, whose rule
refuses partitions.  A failure names the build, the shape, the rank and the first row that differs: the site to look at."""
import numpy as np
import pytest

import rt_amd
from rt_amd import capi
from tests import partition_cases as cases
from tests.test_sky_band_rule import GPU_ROWS, gpu_scene

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A  # alpha byte 0x5A: no finished pixel (every one has alpha 0xFF)
SLACK = 2  # rows allocated beyond rt_hip_padded_local_rows


@pytest.fixture(autouse=True)
def _no_table_outlives_a_test(tracer):
    yield
    tracer.set_emission(None)  # (the session's context is shared: no other test file sees a table)


def assert_rows(got_rgba, got_rgb, want_rgba, want_rgb, rows, what):
    """rows [0, len(rows)) of the rank's buffers against the reference's rows `rows`; the message says how much differs and where first"""
    n = len(rows)
    bad = (got_rgb[:n].view(np.uint32) != want_rgb[rows].view(np.uint32)).any(axis=-1)
    if bad.any():
        local, x = np.argwhere(bad)[0]
        raise AssertionError(f"{what}: the float mean differs in {int(bad.sum())} of {bad.size} pixels ({int(bad.any(axis=1).sum())} of {n} rows); first at local row {local} (image row {rows[local]}), x = {x}: "
                             f"gpu {got_rgb[local, x]} against {want_rgb[rows[local], x]}")
    bad = got_rgba[:n] != want_rgba[rows]
    if bad.any():
        local, x = np.argwhere(bad)[0]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} packed pixels differ; first at local row {local} (image row {rows[local]}), x = {x}: gpu {got_rgba[local, x]:08x} against {want_rgba[rows[local], x]:08x}")


def assert_untouched(got_rgba, got_rgb, got_accum, n, what):
    """every row from `n` on still holds the sentinel"""
    touched = got_rgba[n:] != SENTINEL
    assert not touched.any(), f"{what}: {int(touched.sum())} packed words beyond the rank's {n} rows were written; first at local row {n + int(np.argwhere(touched)[0][0])}"
    touched = ~np.isnan(got_rgb[n:])
    assert not touched.any(), f"{what}: {int(touched.sum())} floats of the mean beyond the rank's {n} rows were written; first at local row {n + int(np.argwhere(touched)[0][0])}"
    if got_accum is not None:
        touched = ~np.isnan(got_accum[n:])
        assert not touched.any(), f"{what}: {int(touched.sum())} floats of the accumulator beyond the rank's {n} rows were written; first at local row {n + int(np.argwhere(touched)[0][0])}"


def expected_variant(name, p, local_rows):
    if name == "preview":  # (not planned: the call reports the preview kernel whether it had rows or not)
        return 4
    assert (p["variant"] == 0) == (local_rows == 0)
    return p["variant"]


def render_share(tracer, name, samples, size, partition, local_rows, padded):
    """One rank's launches into sentinel-filled buffers: (rgba8, float mean, accumulator | None, segments) — the stats of every launch
    held to the plan and to the share's size on the way."""
    import torch

    build = cases.BY_NAME[name]
    width, height = size
    rows = padded + SLACK
    frame = torch.full((rows, width), SENTINEL, dtype=torch.int32, device="cuda:0")
    mean = torch.full((rows, width, 3), float("nan"), dtype=torch.float32, device="cuda:0")
    accum = torch.full((rows, width, 3), float("nan"), dtype=torch.float32, device="cuda:0") if build.passes else None
    stream = torch.cuda.current_stream().cuda_stream
    what = f"{name}, {cases.case_id(name, samples)}, {width} x {height}, partition (rank, world, stripe_rows) = {partition}"
    segments = 0
    plans = cases.plans_of(name, samples, size, local_rows)
    if build.passes:
        for p, (first, after) in zip(plans, cases.pass_windows(samples)):
            tracer.render_pass_device(width, height, first, after - first, accum.data_ptr(), frame.data_ptr(), seed=cases.SEED, flags=build.flags, partition=partition, d_rgb_f32=mean.data_ptr(), stream=stream)
            stats = tracer.stats()
            assert stats["primary_samples"] == local_rows * width * (after - first) and stats["kernel_variant"] == expected_variant(name, p, local_rows), (what, first, stats)
            segments += stats["segments"]
    else:
        tracer.render_device(width, height, frame.data_ptr(), seed=cases.SEED, flags=build.flags, partition=partition, d_rgb_f32=mean.data_ptr(), stream=stream)
        stats = tracer.stats()
        per_pixel = 1 if name == "preview" else samples
        assert stats["primary_samples"] == local_rows * width * per_pixel and stats["kernel_variant"] == expected_variant(name, plans[0], local_rows), (what, stats)
        segments = stats["segments"]
    torch.cuda.synchronize()
    return frame.cpu().numpy().view(np.uint32), mean.cpu().numpy(), accum.cpu().numpy() if accum is not None else None, segments


def check_rank(tracer, name, samples, size, shape, rank, want):
    """-> the rank's segments"""
    world, stripe = shape
    rows = cases.rows_of(size[1], world, stripe, rank)
    padded = cases.padded_rows(size[1], world, stripe)
    what = f"{name}, {cases.case_id(name, samples)}, {size[0]} x {size[1]}, world {world}, stripes of {stripe} rows, rank {rank} ({len(rows)} rows)"
    rgba, rgb, accum, segments = render_share(tracer, name, samples, size, (rank, world, stripe), len(rows), padded)
    if rows:
        assert_rows(rgba, rgb, want[0], want[1], rows, what)
    else:
        assert segments == 0, (what, segments)
    assert_untouched(rgba, rgb, accum, len(rows), what)
    if accum is not None and rows:
        assert np.isfinite(accum[: len(rows)]).all(), what
    return segments


def check_case(tracer, name, samples, size):
    build = cases.BY_NAME[name]
    spp = cases.total_of(samples)
    want = cases.reference(name, spp, size)
    tracer.set_emission(build.table)
    tracer.upload(cases.pod_of(name, spp, size))
    for world, stripe in cases.shapes_of(size):
        counts = cases.row_table(size[1], world, stripe)[1]
        assert rt_amd.padded_local_rows(size[1], world, stripe) == max(counts)
        segments = 0
        for rank in range(world):
            segments += check_rank(tracer, name, samples, size, (world, stripe), rank, want)
            if counts[rank] == 0:  # a render on the same context straight after a launch of nothing is correct
                check_rank(tracer, name, samples, size, (world, stripe), 0, want)
        assert segments == want[2], f"{name}, {cases.case_id(name, samples)}, world {world}, stripes of {stripe} rows: the ranks' segments add up to {segments}, the reference's are {want[2]}"


# ---- the sweep -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,samples", cases.CASES, ids=[cases.case_id(*case) for case in cases.CASES])
def test_every_shape_and_rank_renders_the_references_rows(tracer, name, samples):
    """37 x 29, the ten shapes, every rank: one reference frame, 31 shares (and one more behind every rank without rows)."""
    check_case(tracer, name, samples, cases.FRAME)


@pytest.mark.parametrize("name", [build.name for build in cases.BUILDS])
def test_a_frame_smaller_than_a_tile(tracer, name):
    """5 x 3 under stripes of 1, 2 and 5 rows: every share is a corner of ONE tile, and two of (3, 5)'s three ranks own nothing."""
    check_case(tracer, name, cases.small_frame_samples(cases.BY_NAME[name]), cases.SMALL_FRAME)


def test_shares_that_are_planned_differently_from_their_whole_frame(tracer):
    """1280 x 1024 x 17 samples: the whole frame in 8 x 4 tiles of whole chunks, its shares in 4 x 4 tiles of half chunks
    (tests/test_partition_rows.py holds the plans) — the same pixels."""
    name, samples = cases.LARGE_CASE
    height = cases.LARGE_FRAME[1]
    whole = cases.plan(name, samples, cases.LARGE_FRAME, height)
    share = cases.plan(name, samples, cases.LARGE_FRAME, cases.row_table(height, 2, 8)[1][1])
    assert (whole["halves"], whole["pixels_log2"]) != (share["halves"], share["pixels_log2"])
    check_case(tracer, name, samples, cases.LARGE_FRAME)


# ---- assemble_stripes on its own ---------------------------------------------------------------------------------------------------------
POISON = 0xEE000000  # (a word of a padding row: no rank reaches 0xEE)


def gathered_words(width, height, world, stripe):
    """(gathered uint32[world, padded, width], frame uint32[height, width]): every word of a rank's rows says (rank, local row, x); the
    padding rows are poison; the frame is numpy indexing through the row table"""
    table, counts = cases.row_table(height, world, stripe)
    padded = max(counts)
    x = np.arange(width, dtype=np.uint32)
    gathered = np.full((world, padded, width), POISON, dtype=np.uint32) | x
    for rank in range(world):
        for local in range(counts[rank]):
            gathered[rank, local] = (rank << 24) | (local << 12) | x
    frame = np.stack([gathered[rank, local] for rank, local in table])
    return gathered, frame


@pytest.mark.parametrize("width", [1, 37, 257])  # one word; ragged; more than one block of 256 threads per row
def test_assemble_stripes_alone(tracer, width):
    """rt_hip_assemble_device with no rendering, every shape, into a frame in HBM and into a page-locked host frame."""
    import torch

    height = cases.FRAME[1]
    stream = torch.cuda.current_stream().cuda_stream
    for world, stripe in cases.SHAPES + [(29, 1), (1, 32)]:
        gathered, want = gathered_words(width, height, world, stripe)
        assert not ((want & 0xFF000000) == POISON).any() and len(np.unique(want)) == want.size
        d_gathered = torch.from_numpy(gathered.view(np.int32)).to("cuda:0")
        for host in (False, True):
            frame = torch.full((height + SLACK, width), SENTINEL, dtype=torch.int32, **({"pin_memory": True} if host else {"device": "cuda:0"}))
            tracer.assemble_device(width, height, world, stripe, d_gathered.data_ptr(), frame.data_ptr(), stream)
            torch.cuda.synchronize()
            got = frame.cpu().numpy().view(np.uint32)
            what = f"width {width}, world {world}, stripes of {stripe} rows, {'page-locked host' if host else 'HBM'} frame"
            assert not ((got[:height] & 0xFF000000) == POISON).any(), f"{what}: {int(((got[:height] & 0xFF000000) == POISON).sum())} words of padding rows are in the frame"
            bad = got[:height] != want
            assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} words differ; first at (y, x) = {tuple(np.argwhere(bad)[0])}: {got[:height][bad][0]:08x} against {want[bad][0]:08x} = (rank << 24 | local row << 12 | x)"
            assert (got[height:] == SENTINEL).all(), f"{what}: words beyond the frame's {height} rows were written"


# ---- direct-frame members: frame_rows != 0 -----------------------------------------------------------------------------------------------
MEMBER_BUILDS = [build.name for build in cases.BUILDS if build.members]


def test_the_member_builds_are_what_a_multi_member_context_takes():
    assert MEMBER_BUILDS == ["resident_pinhole", "resident_sm", "bvh_mg", "bvh_device_mg", "boxes_resident", "boxes_bvh", "boxes_tree", "lights_resident", "direct_resident"]


@pytest.mark.parametrize("members", [2, 3, 5])
def test_direct_frame_members_store_every_builds_pixels_to_their_image_rows(members):
    """RT_HIP_MULTI_DIRECT_FRAME into a page-locked back buffer: every member's kernel is launched on (rank, members, 8) with the WHOLE
    frame as its output — output_row = global_row.  The back buffer is filled with the sentinel first, so an unwritten pixel shows."""
    width, height = cases.FRAME
    spp = 20
    counts = cases.row_table(height, members, capi.RT_HIP_DEFAULT_STRIPE_ROWS)[1]
    with rt_amd.HipRayTracer(devices=[0] * members, peer_copy=True, direct_frame=True) as tracer:
        back = np.full((height, width), SENTINEL, dtype=np.uint32)
        for name in MEMBER_BUILDS:
            build = cases.BY_NAME[name]
            want_rgba, _, want_segments = cases.reference(name, spp)
            tracer.set_emission(build.table)
            back[:] = SENTINEL
            _, _, stats = tracer.render(cases.pod_of(name, spp, cases.FRAME), width, height, seed=cases.SEED, flags=build.flags | capi.RT_HIP_FLAG_PERSISTENT_FRAME, out=back)
            what = f"{name}, {members} direct-frame members"
            assert tracer.phases()["transport"] == "direct_frame", (what, tracer.phases())
            bad = back != want_rgba
            unwritten = back == SENTINEL
            assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} packed pixels differ ({int(unwritten.sum())} never written) in image rows {sorted(set(np.argwhere(bad)[:, 0].tolist()))}; "
                                   f"rows of the members: {[cases.rows_of(height, members, 8, r) for r in range(members)]}")
            shares = [tracer.member_stats(r) for r in range(members)]
            assert stats["segments"] == want_segments and sum(s["segments"] for s in shares) == want_segments, (what, stats["segments"], [s["segments"] for s in shares], want_segments)
            assert [s["primary_samples"] for s in shares] == [rows * width * spp for rows in counts], (what, shares)


# ---- the sky band refuses partitions -------------------------------------------------------------------------------------------------------
def test_a_frame_with_a_sky_band_as_a_whole_and_in_shares(monkeypatch, capfd):
    """tests/test_gpu_sky_band.py's "basic" frame at 64 x 40 takes a band of GPU_ROWS rows.  As (0, 1, 5) — a world of one, whatever the
    stripe value — it still does; as rank 0 and rank 1 of (2, 8) the rule refuses and the scene's kernel renders every row of the share.
    All three are the oracle's rows.  The band's own log line (a context created under RT_HIP_SKY_BAND_LOG=1) says which launch took one."""
    import re

    import torch

    from oracle import binding as oracle

    width, height, spp = 64, 40, 17
    band = GPU_ROWS[("basic", height)]
    assert 0 < band < height
    pod = gpu_scene("basic").set_sampling(samples_per_pixel=spp).describe(width, height)
    want_rgba, want_rgb, want_stats = oracle.render(pod, width, height, seed=cases.SEED)
    monkeypatch.setenv("RT_HIP_SKY_BAND_LOG", "1")
    monkeypatch.delenv("RT_HIP_SKY_BAND", raising=False)
    stream = torch.cuda.current_stream().cuda_stream
    with rt_amd.HipRayTracer(device=0) as tracer:
        tracer.upload(pod)
        segments = {}
        for partition, expected_band in (((0, 1, 5), band), ((0, 2, 8), 0), ((1, 2, 8), 0)):
            rank, world, stripe = partition
            rows = cases.rows_of(height, world, stripe, rank)
            padded = cases.padded_rows(height, world, stripe)
            frame = torch.full((padded + SLACK, width), SENTINEL, dtype=torch.int32, device="cuda:0")
            mean = torch.full((padded + SLACK, width, 3), float("nan"), dtype=torch.float32, device="cuda:0")
            capfd.readouterr()
            tracer.render_device(width, height, frame.data_ptr(), seed=cases.SEED, partition=partition, d_rgb_f32=mean.data_ptr(), stream=stream)
            stats = tracer.stats()
            torch.cuda.synchronize()
            logged = [int(found.group(1)) for found in re.finditer(r"rt_hip sky band: rows (\d+) of \d+", capfd.readouterr().err)]
            what = f"sky band frame, partition {partition}"
            assert logged == [expected_band], (what, logged)
            rgba, rgb = frame.cpu().numpy().view(np.uint32), mean.cpu().numpy()
            assert_rows(rgba, rgb, want_rgba, want_rgb, rows, what)
            assert_untouched(rgba, rgb, None, len(rows), what)
            assert stats["primary_samples"] == len(rows) * width * spp and stats["kernel"] == "small", (what, stats)
            segments[partition] = stats["segments"]
        assert segments[(0, 1, 5)] == want_stats["segments"] == segments[(0, 2, 8)] + segments[(1, 2, 8)]
