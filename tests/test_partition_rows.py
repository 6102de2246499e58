"""The partition's row arithmetic on the CPU, held to tests/partition_cases.py's row table — loops written out from include/rt_hip.h's
rule, derived from none of the code under test — for every stripe shape of the GPU sweep (tests/test_gpu_partition_sweep.py):

* rt_hip_local_rows, rt_hip_padded_local_rows and rt_amd.distributed's de-interleave map agree with the table;
* every CPU reference's `partition` argument (the oracle's with both material tables and for the preview, the box, light and
  direct-light restatements') gives the whole reference frame's rows as the table picks them: packed pixels, float mean, and segments
  summed over the ranks.  This is what lets the GPU sweep render ONE whole reference frame per build and sample count;
* invalid partitions are refused;
* the launch plans of the sweep's shares hold what the GPU test relies on — if a change of launch policy empties one of these, a test
  here fails instead of the sweep going quiet."""
import collections

import numpy as np
import pytest

import rt_amd
from oracle import binding as oracle
from rt_amd import distributed
from tests import partition_cases as cases

SIZES = [cases.FRAME, cases.SMALL_FRAME]
SHAPES_AT = [(size, shape) for size in SIZES for shape in cases.shapes_of(size)]


def shape_id(value):
    size, (world, stripe) = value
    return f"{size[0]}x{size[1]}-world{world}-stripe{stripe}"


# ---- the table itself ------------------------------------------------------------------------------------------------------------------
def test_the_row_table_by_hand():
    """A few shapes worked out on paper: the table is the reference of everything else and has no other."""
    table, counts = cases.row_table(29, 3, 7)  # stripes 0-6, 7-13, 14-20, 21-27, 28: ranks 0, 1, 2, 0, 1
    assert counts == [14, 8, 7]
    assert table[0] == (0, 0) and table[6] == (0, 6) and table[7] == (1, 0) and table[14] == (2, 0) and table[21] == (0, 7) and table[27] == (0, 13) and table[28] == (1, 7)
    assert cases.rows_of(29, 3, 7, 1) == [7, 8, 9, 10, 11, 12, 13, 28]  # the last stripe of ONE row
    assert cases.row_table(29, 2, 8)[1] == [16, 13] and cases.rows_of(29, 2, 8, 1) == [8, 9, 10, 11, 12, 13, 14, 15, 24, 25, 26, 27, 28]
    assert cases.row_table(29, 3, 5)[1] == [10, 10, 9] and cases.rows_of(29, 3, 5, 2)[-4:] == [25, 26, 27, 28]
    assert cases.row_table(29, 5, 3)[1] == [6, 6, 6, 6, 5] and cases.rows_of(29, 5, 3, 4) == [12, 13, 14, 27, 28]
    assert cases.row_table(29, 2, 16)[1] == [16, 13]
    assert cases.row_table(29, 2, 32)[1] == [29, 0] and cases.row_table(29, 7, 8)[1] == [8, 8, 8, 5, 0, 0, 0]
    assert cases.rows_of(29, 2, 1, 1) == list(range(1, 29, 2)) and cases.rows_of(29, 4, 2, 3) == [6, 7, 14, 15, 22, 23]
    assert cases.row_table(29, 1, 5) == ([(0, y) for y in range(29)], [29])  # a world of one: the stripe value changes nothing
    assert cases.row_table(3, 3, 5)[1] == [3, 0, 0] and cases.row_table(3, 2, 2)[1] == [2, 1] and cases.rows_of(3, 2, 1, 0) == [0, 2]


@pytest.mark.parametrize("size,shape", SHAPES_AT, ids=[shape_id(v) for v in SHAPES_AT])
def test_every_row_has_one_owner_and_one_place(size, shape):
    world, stripe = shape
    table, counts = cases.row_table(size[1], world, stripe)
    assert len(table) == size[1] and sum(counts) == size[1]
    assert sorted(table) == [(rank, local) for rank in range(world) for local in range(counts[rank])]
    for rank in range(world):
        rows = cases.rows_of(size[1], world, stripe, rank)
        assert rows == sorted(rows) and len(rows) == counts[rank]


# ---- the library's arithmetic ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,shape", SHAPES_AT, ids=[shape_id(v) for v in SHAPES_AT])
def test_the_librarys_rows_are_the_tables(size, shape):
    height, (world, stripe) = size[1], shape
    table, counts = cases.row_table(height, world, stripe)
    assert [rt_amd.local_rows(height, rank, world, stripe) for rank in range(world)] == counts
    assert rt_amd.padded_local_rows(height, world, stripe) == max(counts) == cases.padded_rows(height, world, stripe)
    assert distributed.local_row_table(height, world, stripe).tolist() == [list(entry) for entry in table]
    assert [distributed.owner_and_local_row(y, world, stripe) for y in range(height)] == table
    assert distributed.padded_rows(height, world, stripe) == max(counts)


@pytest.mark.parametrize("rank,world,stripe", [(2, 2, 8), (3, 2, 8), (0, 0, 8), (1, 3, 0), (0, 1, 0)])
def test_invalid_partitions_are_refused(rank, world, stripe):
    """rank >= world, world == 0, stripe_rows == 0 (the render calls' own refusal: tests/test_frame_setup.py)"""
    with pytest.raises(rt_amd.RtHipError) as refused:
        rt_amd.local_rows(29, rank, world, stripe)
    assert refused.value.status == 1 and "invalid partition" in str(refused.value)
    if world == 0 or stripe == 0:  # (rt_hip_padded_local_rows takes no rank)
        with pytest.raises(rt_amd.RtHipError) as refused:
            rt_amd.padded_local_rows(29, world, stripe)
        assert refused.value.status == 1 and "invalid partition" in str(refused.value)


# ---- every reference's partition -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [build.name for build in cases.BUILDS])
def test_a_references_partition_is_the_whole_frames_rows(name):
    """Every build's reference, at the sample count the build renders the small frame with, over every shape of both frames."""
    build = cases.BY_NAME[name]
    spp = cases.total_of(cases.small_frame_samples(build))
    for size in SIZES:
        whole_rgba, whole_rgb, whole_segments = cases.reference(name, spp, size)
        for world, stripe in cases.shapes_of(size):
            segments = 0
            for rank in range(world):
                rows = cases.rows_of(size[1], world, stripe, rank)
                rgba, rgb, stats = cases.reference_render(name, spp, size, partition=(rank, world, stripe))
                what = f"{name} ({build.reference}), {size[0]} x {size[1]}, world {world}, stripes of {stripe}, rank {rank}"
                assert rgba.shape == (len(rows), size[0]) and rgb.shape == (len(rows), size[0], 3), what
                assert np.array_equal(rgba, whole_rgba[rows]), f"{what}: {(rgba != whole_rgba[rows]).sum()} packed pixels differ from the whole frame's rows"
                assert np.array_equal(rgb.view(np.uint32), whole_rgb[rows].view(np.uint32)), f"{what}: the float mean differs from the whole frame's rows"
                assert stats["primary_samples"] == len(rows) * size[0] * (1 if name == "preview" else spp), what
                segments += stats["segments"]
            assert segments == whole_segments, (name, size, world, stripe)


def test_the_references_tell_the_builds_apart():
    """(what makes a frame a test of its build: the sm table, the boxes, the lights and the direct sampling each change the frame)"""
    frame = lambda name: cases.reference(name, 20)[0]
    assert not np.array_equal(frame("resident_sm"), oracle.render(cases.pod_of("resident_sm", 20, cases.FRAME), *cases.FRAME, seed=cases.SEED)[0])
    assert not np.array_equal(frame("bvh_mg"), frame("bvh_sm")) and not np.array_equal(frame("resident_scalar_load"), frame("resident_scalar_load_sm"))
    for name in ("boxes_resident", "boxes_bvh", "boxes_tree", "lights_resident", "lights_bvh"):
        flat = oracle.render(cases.pod_of(name, 20, cases.FRAME), *cases.FRAME, seed=cases.SEED, want_rgb=False)[0]
        assert (frame(name) != flat).mean() > 0.05, name
    assert (frame("direct_resident") != frame("lights_resident")).mean() > 0.05 and (frame("direct_bvh") != frame("lights_bvh")).mean() > 0.05


# ---- the plans the GPU sweep relies on -------------------------------------------------------------------------------------------------
def test_the_build_table_covers_every_family():
    assert [family for family in cases.FAMILIES if any(build.family == family for build in cases.BUILDS)] == cases.FAMILIES
    assert {build.family for build in cases.BUILDS} == set(cases.FAMILIES) and len(cases.BY_NAME) == len(cases.BUILDS)
    for build in cases.BUILDS:
        assert not build.flags & rt_amd.capi.RT_HIP_FLAG_FAST  # (tests/test_gpu_fast_builds.py renders those builds on row shares)


@pytest.mark.parametrize("size", [cases.FRAME, cases.SMALL_FRAME, cases.LARGE_FRAME], ids=lambda size: f"{size[0]}x{size[1]}")
def test_every_share_takes_the_build_its_entry_names(size):
    """... with rows or without: no share is refused, none falls onto another kernel because it is short"""
    shares = 0
    for build, samples, shape, rank, local_rows in cases.every_share(size):
        for p in cases.plans_of(build.name, samples, size, local_rows):
            if p is not None:
                cases.assert_build(build.name, p, local_rows)
                shares += 1
    assert shares > 0


def tile_heights(name):
    """{tile height: [(samples, shape, rank, local_rows)]} over the shares with rows of the build's cases at 37 x 29"""
    seen = collections.defaultdict(list)
    for build, samples, shape, rank, local_rows in cases.every_share():
        if build.name == name and local_rows:
            for p in cases.plans_of(name, samples, cases.FRAME, local_rows):
                seen[cases.tile_height(p)].append((samples, shape, rank, local_rows))
    return seen


TILE_PER_WAVE = [build.name for build in cases.BUILDS if build.tile_per_wave]


@pytest.mark.parametrize("name", TILE_PER_WAVE)
def test_every_tile_per_wave_build_meets_tiles_of_8_4_and_2_rows(name):
    assert set(tile_heights(name)) == {8, 4, 2}, (name, {h: len(v) for h, v in tile_heights(name).items()})


@pytest.mark.parametrize("name", TILE_PER_WAVE)
def test_every_tile_per_wave_build_meets_stripes_and_shares_that_end_inside_a_tile(name):
    """Per tile height: a shape whose stripe_rows is no multiple of it (a tile row spans two stripes: its rows lie apart in the image),
    and a rank whose local_rows is no multiple of it (the last tile row hangs over the share's end)."""
    for height, shares in tile_heights(name).items():
        assert any(world > 1 and stripe % height for _, (world, stripe), _, _ in shares), (name, height)
        assert any(world > 1 and local_rows % height for _, (world, _), _, local_rows in shares), (name, height)
        # ... among them stripes of 1, 3, 5 and 7 rows, and the division branch of global_row (no power of two)
        assert {1, 3, 5, 7} <= {stripe for _, (world, stripe), _, _ in shares if world > 1}, (name, height)


def test_the_rolling_kernels_and_the_preview_meet_every_shape():
    """(no tiles: a share is rows of single pixels — what is left to hold is that every shape and every rank is rendered)"""
    for name in ("tiled", "streamed", "preview"):
        met = {(shape, rank) for build, _, shape, rank, _ in cases.every_share() if build.name == name}
        assert met == {((world, stripe), rank) for world, stripe in cases.SHAPES for rank in range(world)}
    for name in ("tiled", "streamed"):
        chunks = {cases.plan(name, samples, cases.FRAME, rows)["chunks"] for build, samples, _, _, rows in cases.every_share() if build.name == name and rows}
        assert chunks == {1, 2}, (name, chunks)  # 20 samples: a pixel's items meet in HBM, indexed by the share's own rows


def test_a_rank_is_planned_differently_from_its_whole_frame():
    """plan_launch sees the RANK's rows: at 1280 x 1024 x 17 samples the whole frame is cut into 8 x 4 tiles of whole chunks, every share
    of it into 4 x 4 tiles of half chunks — and must render the same pixels."""
    name, spp = cases.LARGE_CASE
    height = cases.LARGE_FRAME[1]
    whole = cases.plan(name, spp, cases.LARGE_FRAME, height)
    assert (whole["halves"], whole["pixels_log2"], cases.tile_height(whole)) == (0, 5, 4), whole
    differing = []
    for world, stripe in cases.LARGE_SHAPES:
        for rank, local_rows in enumerate(cases.row_table(height, world, stripe)[1]):
            p = cases.plan(name, spp, cases.LARGE_FRAME, local_rows)
            if (p["halves"], p["pixels_log2"]) != (whole["halves"], whole["pixels_log2"]):
                differing.append((world, stripe, rank))
                assert (p["halves"], p["pixels_log2"], cases.tile_height(p)) == (1, 4, 4), p
    assert differing == [(2, 8, 0), (2, 8, 1), (3, 5, 0), (3, 5, 1), (3, 5, 2)], differing
    # ... while no share of the small frames is: there the shapes, not the policy, are what varies
    for size in SIZES:
        for build, samples, _, _, local_rows in cases.every_share(size):
            if local_rows and build.name != "preview":
                for p, of_frame in zip(cases.plans_of(build.name, samples, size, local_rows), cases.plans_of(build.name, samples, size, size[1])):
                    assert (p["halves"], p["pixels_log2"], p["tile_w_log2"]) == (of_frame["halves"], of_frame["pixels_log2"], of_frame["tile_w_log2"]), (build.name, samples, local_rows)
