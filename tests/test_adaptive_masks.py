"""tests/adaptive_masks.py on the CPU: the conditions that keep the constructed stop masks of tests/test_gpu_adaptive_masks.py from
hiding a failure, for each of the five tile shapes an adaptive pass of a 37 x 23 frame takes — 8 x 8, 8 x 4, 4 x 4, 4 x 2 and 2 x 2, at
pass sizes 16, 32, 48, 80 and 192 — with the shape asked of the plan dump (tests/adaptive_plan.py), not assumed."""
import numpy as np
import pytest

from tests import adaptive_masks as masks
from tests import adaptive_plan

W, H = 37, 23
SHAPES = [(16, 6), (32, 5), (48, 4), (80, 3), (192, 2)]  # pass size, pixels_log2


@pytest.fixture(scope="module", autouse=True)
def _compiler():
    if adaptive_plan.executable() is None:
        pytest.skip("no g++")


def geometry(size, pixels_log2):
    """The second pass of two of `size` samples through basic.toml's 4 spheres, as tests/test_gpu_adaptive_masks.py runs it."""
    (plan,) = adaptive_plan.plans([(4, 0, 1, W, H, 2 * size, 0, 0, size, size)])
    assert plan["adaptive"] == 1 and plan["pixels_log2"] == pixels_log2, plan
    g = masks.Geometry(W, H, plan["tile_w_log2"], plan["pixels_log2"])
    return plan, g


@pytest.mark.parametrize("size,pixels_log2", SHAPES)
def test_the_geometry_is_the_kernels(size, pixels_log2):
    plan, g = geometry(size, pixels_log2)
    assert g.tile_w * g.tile_h == g.tile_pixels == 1 << pixels_log2
    # every (tile, index) pair names at most one pixel, every pixel has one, and a tile's pixels are its tile_w x tile_h block
    place = g.tile.astype(np.int64) * g.tile_pixels + g.index
    assert len(np.unique(place)) == W * H and g.index.max() == g.tile_pixels - 1 and g.tile.max() == g.tiles_x * g.tiles_y - 1
    for x, y in ((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (17, 11)):
        assert g.tile[y, x] == (y // g.tile_h) * g.tiles_x + x // g.tile_w and g.index[y, x] == (y % g.tile_h) * g.tile_w + x % g.tile_w
    # 37 x 23 hangs over both edges at every shape
    assert W % g.tile_w and H % g.tile_h


@pytest.mark.parametrize("size,pixels_log2", SHAPES)
def test_every_family_is_a_mask_of_the_frame_and_the_controls_are_what_they_say(size, pixels_log2):
    plan, g = geometry(size, pixels_log2)
    made = {family: masks.mask(family, W, H, plan["tile_w_log2"], plan["pixels_log2"]) for family in masks.FAMILIES}
    for family, m in made.items():
        assert m.shape == (H, W) and m.dtype == bool, family
    assert made["all_stopped"].all() and not made["none_stopped"].any()
    assert np.array_equal(made["one_stopped_per_tile"], ~made["one_active_per_tile"])
    assert (~made["corners_only"]).sum() == 4 and not made["corners_only"][[0, 0, -1, -1], [0, -1, 0, -1]].any()
    assert (~made["ragged_edge_only"]).sum() == W + H - 1
    # the checkerboard: every tile is whole, neighbours differ
    board = made["tile_checkerboard"]
    for t in range(g.tiles_x * g.tiles_y):
        assert len(np.unique(board[g.tile == t])) == 1
    assert (board[:, g.tile_w :][:, :: g.tile_w] != board[:, : -g.tile_w][:, :: g.tile_w]).all() and (board[g.tile_h :][:: g.tile_h] != board[: -g.tile_h][:: g.tile_h]).all()


@pytest.mark.parametrize("size,pixels_log2", SHAPES)
def test_random_half_shows_every_mask_bit_both_ways(size, pixels_log2):
    """Every in-tile index occurs at least once stopped and at least once active in some in-frame pixel."""
    plan, g = geometry(size, pixels_log2)
    m = masks.mask("random_half", W, H, plan["tile_w_log2"], plan["pixels_log2"])
    assert 0.4 < m.mean() < 0.6
    for index in range(g.tile_pixels):
        here = m[g.index == index]
        assert here.any() and not here.all(), (index, here)


@pytest.mark.parametrize("size,pixels_log2", SHAPES)
def test_one_per_tile_reaches_every_tile_row_and_column_and_walks_the_index(size, pixels_log2):
    plan, g = geometry(size, pixels_log2)
    active = ~masks.mask("one_active_per_tile", W, H, plan["tile_w_log2"], plan["pixels_log2"])
    in_frame = g.chosen_in_frame()
    assert in_frame.any(axis=1).all() and in_frame.any(axis=0).all(), in_frame
    # the mask has exactly the chosen pixels that the frame holds, one per tile at most
    assert active.sum() == in_frame.sum()
    for t in np.unique(g.tile):
        assert active[g.tile == t].sum() == int(in_frame.flat[t])
        if in_frame.flat[t]:
            assert g.index[active & (g.tile == t)].tolist() == [g.chosen_index(t)]
    # where the frame has at least as many tiles as a tile has pixels, every bit of the mask is the single active pixel of some tile
    if g.tiles_x * g.tiles_y >= g.tile_pixels:
        assert set(g.index[active].tolist()) == set(range(g.tile_pixels))
    assert (g.tiles_x * g.tiles_y >= g.tile_pixels) == (pixels_log2 <= 4)


@pytest.mark.parametrize("size,pixels_log2", SHAPES)
def test_ragged_edge_only_has_silent_tiles_and_tiles_with_all_three_kinds_of_place(size, pixels_log2):
    """At least one tile with no active pixel, and at least one with active, stopped and out-of-frame places together — where the frame
    allows the latter: the 4 x 2 and 2 x 2 tiles keep ONE column and ONE row of a 37 x 23 frame's edge tiles inside it, and those are the
    active ones, so no edge tile of theirs holds a stopped pixel under this family.  There the edge tiles still mix active and
    out-of-frame places, and the three kinds meet under random_half, which the second half of this test asserts for every shape."""
    plan, g = geometry(size, pixels_log2)

    def census(m):
        silent = mixed = active_and_outside = 0
        for t in range(g.tiles_x * g.tiles_y):
            here = m[g.tile == t]
            out_of_frame = g.tile_pixels - here.size
            silent += int(here.all())
            mixed += int(here.any() and not here.all() and out_of_frame > 0)
            active_and_outside += int(not here.all() and out_of_frame > 0)
        return silent, mixed, active_and_outside

    silent, mixed, active_and_outside = census(masks.mask("ragged_edge_only", W, H, plan["tile_w_log2"], plan["pixels_log2"]))
    assert silent >= 1 and active_and_outside == g.tiles_x + g.tiles_y - 1, (silent, active_and_outside)
    possible = W % g.tile_w > 1 or H % g.tile_h > 1  # an edge tile keeps more of the frame than the active column / row
    assert possible == (pixels_log2 >= 4) and (mixed >= 1) == possible, (mixed, possible)
    assert census(masks.mask("random_half", W, H, plan["tile_w_log2"], plan["pixels_log2"]))[1] >= 1


@pytest.mark.parametrize("width,height,tiles", [(64, 16, 16), (128, 32, 64)])
def test_frames_of_whole_8_by_8_tiles(width, height, tiles):
    """The two frames without a ragged edge: at 128 x 32 each of the 64 bit positions is the single active pixel of some tile."""
    (plan,) = adaptive_plan.plans([(4, 0, 1, width, height, 32, 0, 0, 16, 16)])
    assert plan["pixels_log2"] == 6 and plan["tile_w_log2"] == 3, plan
    g = masks.Geometry(width, height, 3, 6)
    assert g.tiles_x * g.tiles_y == tiles and g.chosen_in_frame().all()
    active = ~masks.mask("one_active_per_tile", width, height, 3, 6)
    assert active.sum() == tiles and len(set(g.index[active].tolist())) == min(tiles, 64)
