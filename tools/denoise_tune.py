#!/usr/bin/env python3
"""The table the denoiser's default parameters were chosen from, on the CPU: for basic.toml and dielectric.toml at
96 x 54, the mean squared error of the filtered 16-spp frame against the oracle's 1024-spp float frame, summed over the two scenes,
for a small grid around the starting point (iterations 4, squarings 5, sigmas 0.6 / 0.1 / 0.05).  The filter is the CPU restatement
(tests/native/denoise_reference.cpp), which the device equals bit for bit; no GPU is involved.

    python tools/denoise_tune.py            # prints the table, best row last
"""
import itertools
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import rt_amd  # noqa: E402
from oracle import binding as oracle  # noqa: E402
from tests import denoise_reference as ref  # noqa: E402

W, H, SEED = 96, 54, 7


def frames(name):
    noisy = oracle.render(rt_amd.Scene.named(name).set_sampling(16).describe(W, H), W, H, seed=SEED)[1]
    truth = oracle.render(rt_amd.Scene.named(name).set_sampling(1024).describe(W, H), W, H, seed=SEED + 1)[1]
    guide = ref.compose_guide(rt_amd.Scene.named(name).describe(W, H), W, H)
    return noisy, truth.astype(np.float64), guide


def mse(a, truth):
    return float(np.mean((a.astype(np.float64) - truth) ** 2))


def main():
    scenes = {name: frames(name) for name in ("basic", "dielectric")}
    print("unfiltered: " + ", ".join(f"{name} {mse(noisy, truth):.6f}" for name, (noisy, truth, _) in scenes.items()))
    rows = []
    grid = itertools.product((1, 2, 4), (3, 5), (0.1, 0.2, 0.6), (0.1,), (0.02, 0.05))
    for iterations, squarings, colour, albedo, depth in grid:
        p = ref.params(iterations=iterations, normal_squarings=squarings, sigma_colour=colour, sigma_albedo=albedo, sigma_depth=depth)
        errors = [mse(ref.filter(noisy, guide, p)[0], truth) for noisy, truth, guide in scenes.values()]
        rows.append((sum(errors), iterations, squarings, colour, albedo, depth, *errors))
    rows.sort(reverse=True)
    print(f"{'sum':>9s} {'iter':>4s} {'sq':>2s} {'colour':>6s} {'albedo':>6s} {'depth':>5s} {'basic':>9s} {'dielectric':>10s}")
    for total, iterations, squarings, colour, albedo, depth, basic, dielectric in rows:
        print(f"{total:9.6f} {iterations:4d} {squarings:2d} {colour:6.2f} {albedo:6.2f} {depth:5.2f} {basic:9.6f} {dielectric:10.6f}")


if __name__ == "__main__":
    main()
