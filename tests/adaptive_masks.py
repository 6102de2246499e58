"""Constructed stop masks for the adaptive builds of the render kernels.  An adaptive wave ballots its tile's state words
into one 64-bit mask and indexes it by a pixel's PLACE in the tile, which depends on the tile shape the plan chose; the masks here are
built from that geometry — the kernel's: tiles anchored at pixel (0, 0), pixel (x, y) in tile (x // tw, y // th) at in-tile index
(y % th) * tw + x % tw, with tw = 1 << tile_w_log2 and th = (1 << pixels_log2) >> tile_w_log2, as the dump of tests/adaptive_plan.py
reports them.  Every family is a bool[height, width], True = stopped.  TEST INFRASTRUCTURE, CPU only: tests/test_adaptive_masks.py
pins what keeps these masks from hiding a failure, tests/test_gpu_adaptive_masks.py sets them between two passes."""
import numpy as np

FAMILIES = ("all_stopped", "none_stopped", "one_active_per_tile", "one_stopped_per_tile", "random_half", "ragged_edge_only", "corners_only", "tile_checkerboard")
# random_half's seed: chosen so that at 37 x 23 every in-tile index of each of the five tile shapes occurs stopped AND active inside the
# frame (tests/test_adaptive_masks.py asserts it; with 8 pixels at some indices of the 8 x 8 tile about every second seed fails)
RANDOM_SEED = 3


class Geometry:
    """Where every pixel of a width x height frame lies in the tiles of one plan."""

    def __init__(self, width, height, tile_w_log2, pixels_log2):
        assert 0 <= tile_w_log2 <= pixels_log2 <= 6, (tile_w_log2, pixels_log2)
        self.width, self.height = width, height
        self.tile_w, self.tile_h = 1 << tile_w_log2, (1 << pixels_log2) >> tile_w_log2
        self.tile_pixels = 1 << pixels_log2
        self.tiles_x, self.tiles_y = -(-width // self.tile_w), -(-height // self.tile_h)
        y, x = np.mgrid[0:height, 0:width]
        self.tile_x, self.tile_y = x // self.tile_w, y // self.tile_h
        self.tile = self.tile_y * self.tiles_x + self.tile_x  # row-major over tiles
        self.index = (y % self.tile_h) * self.tile_w + x % self.tile_w  # the bit of the wave's mask

    def chosen_index(self, tile):
        """The in-tile index one_active_per_tile and one_stopped_per_tile single out in tile number `tile`."""
        return (7 * tile + 3) % self.tile_pixels

    def chosen_in_frame(self):
        """bool[tiles_y, tiles_x]: the tile's chosen pixel lies inside the frame."""
        tile = np.arange(self.tiles_x * self.tiles_y).reshape(self.tiles_y, self.tiles_x)
        index = self.chosen_index(tile)
        x = (tile % self.tiles_x) * self.tile_w + index % self.tile_w
        y = (tile // self.tiles_x) * self.tile_h + index // self.tile_w
        return (x < self.width) & (y < self.height)


def mask(family, width, height, tile_w_log2, pixels_log2):
    g = Geometry(width, height, tile_w_log2, pixels_log2)
    if family == "all_stopped":
        return np.ones((height, width), dtype=bool)
    if family == "none_stopped":
        return np.zeros((height, width), dtype=bool)
    if family == "one_active_per_tile":  # (a tile whose chosen pixel falls outside the frame is left all-stopped)
        return g.index != g.chosen_index(g.tile)
    if family == "one_stopped_per_tile":
        return g.index == g.chosen_index(g.tile)
    if family == "random_half":
        return np.random.default_rng(RANDOM_SEED).random((height, width)) < 0.5
    if family == "ragged_edge_only":  # only the last column and the last row are active
        stopped = np.ones((height, width), dtype=bool)
        stopped[-1, :] = stopped[:, -1] = False
        return stopped
    if family == "corners_only":
        stopped = np.ones((height, width), dtype=bool)
        stopped[0, 0] = stopped[0, -1] = stopped[-1, 0] = stopped[-1, -1] = False
        return stopped
    if family == "tile_checkerboard":  # whole tiles alternate, tile (0, 0) stopped
        return (g.tile_x + g.tile_y) % 2 == 0
    raise ValueError(family)
