#!/usr/bin/env python3
"""Write the fixture of RT_HIP_FLAG_THIN_LENS:

    tests/golden/lens_64x36_spp20.npz   basic.toml through its axis-aligned camera and the lens aperture=0.06,focus=3.4, both scatter
                                        tables, through the CPU restatement of the lens contract (tests/native/lens_reference.cpp: the
                                        oracle with a sample loop that knows a lens): rgba, rgba_sm, rgb, rgb_sm, segments, segments_sm,
                                        seed, spp, max_bounces, aperture_radius, focus_distance

and confirm, with the restatement, what tests/test_gpu_lens.py asks of the scene: the lens frame differs from the flag-less one in more
than 20 percent of the pixels.  Regenerate only together with a change of the contract."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from oracle import binding as oracle  # noqa: E402
from tests import lens_reference as lens_ref  # noqa: E402

OUT = ROOT / "tests" / "golden"
width, height, spp, bounces, seed = 64, 36, 20, 8, 23
lens = (0.06, 3.4)
pod = lens_ref.named_scene("basic", lens_ref.AXIS_CAMERA, spp, bounces).describe(width, height)
rgba, rgb, stats = lens_ref.render(pod, width, height, lens, seed=seed)
rgba_sm, rgb_sm, stats_sm = lens_ref.render(pod, width, height, lens, seed=seed, sm_materials=True)
np.savez_compressed(OUT / "lens_64x36_spp20.npz", width=width, height=height, spp=spp, max_bounces=bounces, seed=seed, aperture_radius=np.float32(lens[0]), focus_distance=np.float32(lens[1]), rgba=rgba, rgb=rgb,
                    segments=stats["segments"], rgba_sm=rgba_sm, rgb_sm=rgb_sm, segments_sm=stats_sm["segments"])
print("lens_64x36_spp20", stats, stats_sm)
for sm, blurred in ((False, rgba), (True, rgba_sm)):
    sharp, _, _ = oracle.render(pod, width, height, seed=seed, want_rgb=False, sm_materials=sm)
    share = float((blurred != sharp).mean())
    print(f"pixels that differ from the flag-less frame ({'sm' if sm else 'mg'} table): {100 * share:.1f} percent")
    assert share > 0.2
