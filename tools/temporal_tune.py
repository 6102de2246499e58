#!/usr/bin/env python3
"""The table temporal accumulation's default parameters were chosen from, on the CPU: for basic.toml and
dielectric.toml at 96 x 54, eight oracle frames of 16 spp with seeds of their own are blended by the CPU restatement
(tests/native/reproject_reference.cpp, which the device equals bit for bit), once with the camera at rest and once on a dolly of eight
steps; the figure is the mean squared error of the last blended frame against the oracle's 1024-spp frame of the last camera, summed
over scenes and sequences.  No GPU is involved.

    python tools/temporal_tune.py            # prints the table, best row last
"""
import itertools
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import rt_amd  # noqa: E402
from oracle import binding as oracle  # noqa: E402
from tests import denoise_reference as guide_ref  # noqa: E402
from tests import reproject_reference as ref  # noqa: E402

W, H, FRAMES, SPP = 96, 54, 8, 16
CAMERAS = {"basic": (0.0, 1.0, 3.0), "dielectric": (0.0, 1.0, 7.0)}  # the scenes' own positions; both look along -z
DOLLY = {"basic": 0.07, "dielectric": 0.14}  # world units along +x per frame: seven steps cross more than a tenth of the frame's width


def camera(name, step, moving):
    x, y, z = CAMERAS[name]
    return (x + (DOLLY[name] * step if moving else 0.0), y, z), (0.0, 0.0, -1.0)


def sequence_inputs(name, moving):
    """[(scene pod, guide, 16-spp mean, 16)] for the eight frames, and the 1024-spp frame of the last camera."""
    frames = []
    for step in range(FRAMES):
        scene = rt_amd.Scene.named(name).set_camera(*camera(name, step, moving))
        pod = scene.set_sampling(SPP).describe(W, H)
        frames.append((pod, guide_ref.compose_guide(pod, W, H), oracle.render(pod, W, H, seed=1 + step)[1], SPP))
    truth = oracle.render(rt_amd.Scene.named(name).set_camera(*camera(name, FRAMES - 1, moving)).set_sampling(1024).describe(W, H), W, H, seed=100)[1]
    return frames, truth.astype(np.float64)


def shift_in_pixels(frames):
    """How far the first camera's view of the last frame's surface points lies from where they are now: the median over hit pixels."""
    first, last = frames[0], frames[-1]
    ramp = np.zeros((H, W, 3), dtype=np.float32)
    ramp[..., 0], ramp[..., 1] = np.arange(W)[None, :], np.arange(H)[:, None]
    start = ref.frame(first[0], first[1], ramp, SPP)
    moved = ref.frame(last[0], last[1], np.zeros_like(ramp), 1, ref.matrix_of(first[0]), start[0], start[1], ref.params(max_history_samples=1 << 20, position_tolerance=0.05))
    had = moved[1][..., 3] > 1.0
    dx = moved[0][..., 0][had] * (SPP + 1) / SPP - np.broadcast_to(np.arange(W)[None, :], (H, W))[had]
    return float(np.median(np.abs(dx)))


def mse(a, truth):
    return float(np.mean((a.astype(np.float64) - truth) ** 2))


def main():
    cases = {(name, moving): sequence_inputs(name, moving) for name in ("basic", "dielectric") for moving in (False, True)}
    for (name, moving), (frames, truth) in cases.items():
        line = f"{name:10s} {'dolly' if moving else 'rest':5s}: last 16-spp frame alone {mse(frames[-1][2], truth):.6f}"
        if moving:
            line += f", the dolly moves the view by {shift_in_pixels(frames):.1f} pixels (a tenth of the width: {W / 10:.1f})"
        print(line)
    rows = []
    for cap, tolerance, threshold in itertools.product((16, 32, 48, 64, 128, 1024), (0.002, 0.01, 0.05), (0.5, 0.9, 0.99)):
        p = ref.params(max_history_samples=cap, position_tolerance=tolerance, normal_threshold=threshold)
        errors = [mse(ref.sequence(frames, p)[-1][0], truth) for frames, truth in cases.values()]
        rows.append((sum(errors), cap, tolerance, threshold, *errors))
    rows.sort(reverse=True)
    print(f"{'sum':>9s} {'cap':>5s} {'tol':>6s} {'normal':>6s} " + " ".join(f"{name[:5] + ('/dolly' if moving else '/rest'):>11s}" for name, moving in cases))
    for total, cap, tolerance, threshold, *errors in rows:
        print(f"{total:9.6f} {cap:5d} {tolerance:6.3f} {threshold:6.2f} " + " ".join(f"{e:11.6f}" for e in errors))


if __name__ == "__main__":
    main()
