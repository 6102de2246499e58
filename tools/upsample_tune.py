#!/usr/bin/env python3
"""The table guided upsampling's default min_weight was chosen from, on the CPU: for basic.toml, basic_plane.toml and
tests/golden/scenes/boxes.toml (boxes traced) at 96 x 54, the mean squared error of the frame rebuilt from a 16-spp frame traced at
factor 2, 3 and 4 against the oracle's own full-size 1024-spp float frame, per min_weight, the other parameters at the denoiser's
defaults; with it the orphans each threshold makes.  min_weight = 1 with every tap of one surface is the plain bilinear frame wherever
a tap disagrees at all: the row to beat.  The reconstruction is the CPU restatement (tests/native/upsample_reference.cpp), which the
device equals bit for bit; no GPU is involved.  A record, not a gate.

    python tools/upsample_tune.py            # prints the table
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import rt_amd  # noqa: E402
from oracle import binding as oracle  # noqa: E402
from tests import box_reference  # noqa: E402
from tests import denoise_reference  # noqa: E402
from tests import upsample_reference as ref  # noqa: E402

W, H, SEED = 96, 54, 7
SCENES = {
    "basic": (lambda spp: rt_amd.Scene.named("basic").set_sampling(spp).describe(W, H), False),
    "planes": (lambda spp: rt_amd.Scene.named("basic_plane").set_sampling(spp).describe(W, H), False),
    "boxes": (lambda spp: rt_amd.Scene.load(ROOT / "tests" / "golden" / "scenes" / "boxes.toml").set_sampling(spp).describe(W, H), True),
}
MIN_WEIGHTS = [1.0, 0.25, 2.0**-4, 2.0**-6, 2.0**-8, 2.0**-10, 2.0**-14, 1e-6]


def mse(a, truth):
    return float(np.mean((a.astype(np.float64) - truth) ** 2))


def main():
    cases = []
    for name, (make, boxes) in SCENES.items():
        render = box_reference.render if boxes else oracle.render
        truth = render(make(1024), W, H, seed=SEED + 1)[1].astype(np.float64)
        whole = render(make(16), W, H, seed=SEED)[1]
        guide_full = denoise_reference.compose_guide(make(16), W, H, boxes=boxes)
        print(f"{name}: the traced 16-spp full frame {mse(whole, truth):.6f}")
        for factor in (2, 3, 4):
            w, h = -(-W // factor), -(-H // factor)
            low = render(make(16), w, h, seed=SEED)[1]  # (the full frame's matrix at the low size: the same view)
            guide_low = denoise_reference.compose_guide(make(16), w, h, boxes=boxes)
            cases.append((name, factor, low, guide_low, guide_full, truth))
    print(f"{'min_weight':>12s} " + " ".join(f"{name[:6]}/{factor}" for name, factor, *_ in cases) + "       sum   orphans")
    for min_weight in MIN_WEIGHTS:
        errors, orphans = [], 0
        for _, _, low, guide_low, guide_full, truth in cases:
            out, _, n = ref.frame(low, guide_low, guide_full, ref.params(min_weight=min_weight))
            errors.append(mse(out, truth))
            orphans += n
        print(f"{min_weight:12.3e} " + " ".join(f"{e:8.6f}" for e in errors) + f"  {sum(errors):8.6f}  {orphans:8d}")


if __name__ == "__main__":
    main()
