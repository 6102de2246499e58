#!/usr/bin/env python3
"""How far the frames of tools/upscale_bench.py lie from the truth, on scenes/basic.toml at 1920x1080:

    python tools/upscale_quality.py > profiles/r24/upscale_quality.jsonl

One JSON line per frame: the mean squared error of its float mean against a full-size 4096-spp frame (another seed) — the whole
16-spp frame, and the frames rt_hip_render_upscaled rebuilds at factors 2, 3 and 4, each from the same spp (16) and from factor^2 x
the spp (the whole frame's ray budget) — with the orphans.  Every frame is rendered once, on the
GPU; the errors are computed on the host in binary64.  A record: nothing in the header or in DESIGN.md promises a quality."""
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

WIDTH, HEIGHT, SEED, SPP, TRUTH_SPP = 1920, 1080, 1, 16, 4096


def main():
    import rt_amd

    def pod(spp):
        return rt_amd.Scene.named("basic").set_sampling(spp).describe(WIDTH, HEIGHT)

    def mse(a, truth):
        return float(np.mean((a.astype(np.float64) - truth) ** 2))

    with rt_amd.HipRayTracer(device=0) as tracer:
        truth = tracer.render(pod(TRUTH_SPP), WIDTH, HEIGHT, seed=SEED + 1000, want_rgb=True)[1].astype(np.float64)
        whole = tracer.render(pod(SPP), WIDTH, HEIGHT, seed=SEED, want_rgb=True)[1]
        print(json.dumps({"case": "whole", "spp": SPP, "truth_spp": TRUTH_SPP, "mse": mse(whole, truth)}), flush=True)
        for factor in (2, 3, 4):
            for spp in (SPP, SPP * factor * factor):
                _, rgb, _, info = tracer.render_upscaled(pod(spp), WIDTH, HEIGHT, seed=SEED, factor=factor, want_rgb=True)
                print(json.dumps({"case": f"upscaled:{factor}:{spp}", "factor": factor, "spp": spp, "truth_spp": TRUTH_SPP, "mse": mse(rgb, truth), **info}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
