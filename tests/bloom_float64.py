"""Bloom a second time, in float64 numpy, written from the TEXT of DESIGN.md §3.16 — the level rule, the bright pass, the three tap
rules with their clamped indices, the composite — and not from rt_amd/csrc/bloom_rules.hpp: whole-image index arrays instead of per-texel
rules, sums in whatever order numpy takes them.  TEST INFRASTRUCTURE (tests/test_bloom_independent.py, tests/test_bloom_rules.py).

Beside every image it carries a MAGNITUDE image: the same linear filters over the sanitised channels instead of the bright ones.  The
bright pass scales a channel by at most 1 and everything after it is a sum with non-negative weights of non-negative values, so the
magnitude image bounds every operand on a texel's way — the scale a rounding error is relative to."""
from __future__ import annotations

import numpy as np

CAP = 2.0 ** 20
BINOMIAL = (1.0, 4.0, 6.0, 4.0, 1.0)


def level_sizes(width: int, height: int, levels: int):
    sizes, w, h = [], width, height
    while len(sizes) < levels:
        w, h = -(-w // 2), -(-h // 2)
        sizes.append((w, h))
        if (w, h) == (1, 1):
            break
    return sizes


def sanitised(rgb):
    c = np.asarray(rgb, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.where((c == c) & (c > 0), np.minimum(c, CAP), 0.0)


def bright_pass(s, threshold: float, knee: float):
    m = s.max(axis=-1)
    rq = np.clip(m - (threshold - knee), 0.0, 2.0 * knee)
    soft = rq * rq / (4.0 * knee) if knee > 0 else np.zeros_like(m)
    w = np.maximum(np.maximum(soft, m - threshold), 0.0)
    scale = np.divide(w, m, out=np.zeros_like(m), where=m > 0)
    return s * scale[..., None]


def prefilter(b):
    H, W = b.shape[:2]
    X, Y = np.arange(-(-W // 2)), np.arange(-(-H // 2))
    x0, x1, y0, y1 = np.minimum(2 * X, W - 1), np.minimum(2 * X + 1, W - 1), np.minimum(2 * Y, H - 1), np.minimum(2 * Y + 1, H - 1)
    return (b[y0][:, x0] + b[y0][:, x1] + b[y1][:, x0] + b[y1][:, x1]) * 0.25


def down(level):
    h, w = level.shape[:2]
    X, Y = np.arange(-(-w // 2)), np.arange(-(-h // 2))
    rows = sum(weight * level[:, np.clip(2 * X + k - 2, 0, w - 1)] for k, weight in enumerate(BINOMIAL))
    return sum(weight * rows[np.clip(2 * Y + k - 2, 0, h - 1)] for k, weight in enumerate(BINOMIAL)) / 256.0


def tent(coarse, width: int, height: int):
    hc, wc = coarse.shape[:2]
    x, y = np.arange(width), np.arange(height)
    X, Y = x >> 1, y >> 1
    Xn = np.where(x & 1, np.minimum(X + 1, wc - 1), np.maximum(X - 1, 0))
    Yn = np.where(y & 1, np.minimum(Y + 1, hc - 1), np.maximum(Y - 1, 0))
    rows = 0.75 * coarse[:, X] + 0.25 * coarse[:, Xn]
    return 0.75 * rows[Y] + 0.25 * rows[Yn]


def layer_of(b, n_levels: int, scatter: float):
    """bright image -> (the glow layer at full size, the levels on the way down)."""
    H, W = b.shape[:2]
    levels = [prefilter(b)]
    for _ in range(n_levels - 1):
        levels.append(down(levels[-1]))
    up = levels[-1]
    for i in range(n_levels - 2, -1, -1):
        up = levels[i] + scatter * tent(up, levels[i].shape[1], levels[i].shape[0])
    return tent(up, W, H), levels


def bloom(rgb, threshold: float, knee: float, intensity: float, scatter: float, levels: int):
    """-> dict: out, layer, their magnitude images out_scale and layer_scale, the levels on the way down, n (the level count), gain.
    The parameters are taken as the float32 values the device is handed, widened."""
    threshold, knee, intensity, scatter = (float(np.float32(v)) for v in (threshold, knee, intensity, scatter))
    rgb = np.asarray(rgb, dtype=np.float64)
    H, W = rgb.shape[:2]
    n = len(level_sizes(W, H, levels))
    s = sanitised(rgb)
    layer, down_levels = layer_of(bright_pass(s, threshold, knee), n, scatter)
    layer_scale, _ = layer_of(s, n, scatter)
    gain = intensity / sum(scatter ** i for i in range(n))
    return {"out": rgb + gain * layer, "layer": layer, "out_scale": np.abs(rgb) + gain * layer_scale, "layer_scale": layer_scale, "levels": down_levels, "n": n, "gain": gain}
