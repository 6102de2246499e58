"""Guided upsampling in numpy float64, written from DESIGN.md §3.14 — and §3.8 for the three weight terms it shares with the denoiser —
and from nothing else: a second reading of the contract beside the float32 restatement over rt_amd/csrc/upsample_rules.hpp
(tests/upsample_reference.py).  TEST INFRASTRUCTURE.  Whole-image index arrays, float64 geometry from u = ((2x + 1) w − W) / (2W) with
numpy's floor, numpy's own summation over the four taps: nothing of the header's order of operations is kept, so a slip in the header
(a sigma unsquared, the depth term over the shallower hit, a normal term applied to sky) does not pass for the contract.

§3.14 in the order it is read here:
  geometry  full pixel x has its centre at u in low-pixel coordinates; X0 = floor(u), X1 = X0 + 1, bx1 = u − X0, bx0 = 1 − bx1; y likewise
  taps      (X0 | X1, Y0 | Y1); a tap outside the low frame is skipped
  weight    b = bx · by, times — between two hits — max(0, n_p · n_q) squared `normal_squarings` times,
            1 / (1 + (Δz / (sigma_depth · max(z_p, z_q)))²) and 1 / (1 + |Δa|² / sigma_albedo²); sky against hit 0, sky against sky b alone;
            a weight that comes out as NaN is 0; a tap with a non-finite colour channel has weight 0 and colour 0
  pixel     sw = Σ w;  sw ≥ min_weight and sw > 0:  Σ w c / sw;  otherwise an orphan:  Σ b c / Σ b over the in-frame taps with a finite
            colour, or (0, 0, 0) where Σ b is not positive"""
from __future__ import annotations

import numpy as np

F64 = np.float64


def _axis(full: int, low: int):
    """(index of the first tap int64[full], weight of the first tap, weight of the second)."""
    x = np.arange(full, dtype=F64)
    u = ((2.0 * x + 1.0) * low - full) / (2.0 * full)
    first = np.floor(u)
    second_weight = u - first
    return first.astype(np.int64), 1.0 - second_weight, second_weight


def frame(rgb_low, guide_low, guide_full, normal_squarings: int, sigma_albedo: float, sigma_depth: float, min_weight: float) -> dict:
    """rgb_low [h, w, 3], guide_low [h, w, 8], guide_full [H, W, 8] (float32 records, the id's bits in word 7) ->
    {"out": float64[H, W, 3], "sw": float64[H, W] the guided weight sum, "orphan": bool[H, W], "scale": float64[H, W, 3] the same sums
    over |c|, "orphans": their count}."""
    ids_low = np.ascontiguousarray(np.asarray(guide_low, dtype=np.float32)[..., 7]).view(np.uint32)
    ids_full = np.ascontiguousarray(np.asarray(guide_full, dtype=np.float32)[..., 7]).view(np.uint32)
    low, gl, gf = np.asarray(rgb_low, dtype=F64), np.asarray(guide_low, dtype=F64), np.asarray(guide_full, dtype=F64)
    h, w = low.shape[:2]
    H, W = gf.shape[:2]
    x0, bx0, bx1 = _axis(W, w)
    y0, by0, by1 = _axis(H, h)
    sky_p = ids_full == 0

    weights, plain, colours = [], [], []
    with np.errstate(all="ignore"):
        for j, by in ((0, by0), (1, by1)):
            for i, bx in ((0, bx0), (1, bx1)):
                qx, qy = x0 + i, y0 + j
                inside = ((qy >= 0) & (qy < h))[:, None] & ((qx >= 0) & (qx < w))[None, :]
                at = (np.clip(qy, 0, h - 1)[:, None], np.clip(qx, 0, w - 1)[None, :])
                q, c, sky_q = gl[at], low[at], (ids_low == 0)[at]
                b = by[:, None] * bx[None, :]
                along = np.maximum(0.0, (gf[..., 0:3] * q[..., 0:3]).sum(axis=-1))
                normal = along ** float(2 ** normal_squarings)
                depth = 1.0 / (1.0 + ((gf[..., 3] - q[..., 3]) / (sigma_depth * np.maximum(gf[..., 3], q[..., 3]))) ** 2)
                albedo = 1.0 / (1.0 + ((gf[..., 4:7] - q[..., 4:7]) ** 2).sum(axis=-1) / sigma_albedo**2)
                hits = ~sky_p & ~sky_q
                guided = np.where(hits, b * normal * depth * albedo, b)
                finite = np.isfinite(c).all(axis=-1)
                usable = inside & (sky_p == sky_q) & finite & ~np.isnan(guided)
                weights.append(np.where(usable, guided, 0.0))
                plain.append(np.where(inside & finite, b, 0.0))
                colours.append(np.where(finite[..., None], c, 0.0))
    weights, plain, colours = np.stack(weights), np.stack(plain), np.stack(colours)
    sw, sb = weights.sum(axis=0), plain.sum(axis=0)
    is_guided = (sw >= min_weight) & (sw > 0.0)
    has_plain = sb > 0.0
    with np.errstate(all="ignore"):
        by_guide = lambda values: (weights[..., None] * values).sum(axis=0) / sw[..., None]  # noqa: E731
        by_plain = lambda values: (plain[..., None] * values).sum(axis=0) / sb[..., None]  # noqa: E731
        pick = lambda values: np.where(is_guided[..., None], by_guide(values), np.where(has_plain[..., None], by_plain(values), 0.0))  # noqa: E731
        out, scale = pick(colours), pick(np.abs(colours))
    return {"out": out, "sw": sw, "orphan": ~is_guided, "scale": scale, "orphans": int((~is_guided).sum())}
