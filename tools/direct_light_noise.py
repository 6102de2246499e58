#!/usr/bin/env python3
"""The noise of the two estimators, on the CPU through the two restatements: tests/golden/scenes/lights.toml at 64x36x64
over 16 seeds, RT_HIP_FLAG_EMISSION alone (tests/native/light_reference.cpp) against RT_HIP_FLAG_DIRECT_LIGHT
(tests/native/direct_reference.cpp).  For the floor pixels the lamp lights — the primary ray of the pixel centre hits the ground plane and
the direct frame's across-seed mean is brighter than the sky alone makes any floor pixel — the across-seed variance of the float mean,
each estimator against ITS OWN mean: the two converge to different images, so no mean is compared with the other's.

    python tools/direct_light_noise.py > profiles/r23/noise.txt"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from oracle import binding as oracle  # noqa: E402
from tests import direct_reference as direct_ref  # noqa: E402
from tests import light_reference as light_ref  # noqa: E402

WIDTH, HEIGHT, SPP, SEEDS = 64, 36, 64, 16


def main():
    pod = light_ref.lights_scene(spp=SPP).describe(WIDTH, HEIGHT)
    rays = [oracle.primary_ray(pod, WIDTH, HEIGHT, x, y) for y in range(HEIGHT) for x in range(WIDTH)]
    _, kind, _, _ = oracle.closest_hit(pod, np.array([r[0] for r in rays]), np.array([r[1] for r in rays]))
    floor = (kind == 2).reshape(HEIGHT, WIDTH)
    implicit = np.stack([light_ref.render(pod, WIDTH, HEIGHT, light_ref.LIGHTS_TABLE, seed=s)[1] for s in range(1, SEEDS + 1)]).astype(np.float64)
    direct = np.stack([direct_ref.render(pod, WIDTH, HEIGHT, light_ref.LIGHTS_TABLE, seed=s)[1] for s in range(1, SEEDS + 1)]).astype(np.float64)
    unlit = np.stack([direct_ref.render(pod, WIDTH, HEIGHT, None, seed=s)[1] for s in range(1, SEEDS + 1)]).astype(np.float64)
    lit = floor & ((direct.mean(axis=0) - unlit.mean(axis=0)).sum(axis=2) > 0.1)  # the lamp adds at least 0.1 to r + g + b
    print(f"lights.toml {WIDTH}x{HEIGHT}x{SPP}, {SEEDS} seeds; floor pixels {int(floor.sum())}, of them lamp-lit {int(lit.sum())}")
    for name, frames in (("RT_HIP_FLAG_EMISSION", implicit), ("RT_HIP_FLAG_EMISSION | RT_HIP_FLAG_DIRECT_LIGHT", direct)):
        variance = frames.var(axis=0, ddof=1)[lit]  # per pixel and channel, against the estimator's own across-seed mean
        mean = frames.mean(axis=0)[lit]
        print(f"{name}: mean of the lamp-lit floor {mean.mean():.4f}, mean across-seed variance {variance.mean():.3e}, median {np.median(variance):.3e}, relative standard deviation {np.sqrt(variance.mean()) / mean.mean():.4f}")


if __name__ == "__main__":
    main()
