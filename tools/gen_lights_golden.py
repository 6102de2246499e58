#!/usr/bin/env python3
"""Write the two fixtures of RT_HIP_FLAG_EMISSION:

    tests/golden/scenes/lights.toml       this project's own scene: a ground plane, a lamp sphere, one sphere per scatter function
    tests/golden/lights_64x36_spp20.npz   its frame under the table "lamp=4,3.2,2", both scatter tables, through the CPU restatement of
                                          the light contract (tests/native/light_reference.cpp: the oracle with a trace loop that knows
                                          lights): rgba, rgba_sm, rgb, rgb_sm, segments, segments_sm, seed, spp, max_bounces, emission

and confirm, with the restatement, what tests/test_gpu_lights.py asks of the scene: the lit frame differs from the flag-less one in more
than 5 percent of the pixels.  Regenerate only together with a change of the contract."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

LIGHTS_TOML = """\
# tests/golden/scenes/lights.toml — this project's own scene for RT_HIP_FLAG_EMISSION (DESIGN.md §3.12): the ground plane, a lamp
# sphere hanging over it, and one sphere per scatter function (lambert, metal, dielectric — the last one refracts under the sm table
# and is lambert under mg's).  The materials are NAMED: the emission table of the fixture is the spec "lamp=4,3.2,2"
# (rt_hip_lights_from_spec; rt_headless --light lamp=4,3.2,2).  Without the flag the lamp is a grey lambert sphere.
# Written by tools/gen_lights_golden.py.

samples_per_pixel = 64
max_bounces = 8

camera = { position = [0.3, 1.5, 5.0], direction = [0, -0.1, -1] }

materials = [
    { name = 'ground', type = 'lambert',    albedo = [0.55, 0.55, 0.5] },
    { name = 'lamp',   type = 'lambert',    albedo = [0.7, 0.7, 0.7] },
    { name = 'clay',   type = 'lambert',    albedo = [0.8, 0.3, 0.25] },
    { name = 'brass',  type = 'metal',      albedo = [0.9, 0.85, 0.7], roughness = 0.1 },
    { name = 'glass',  type = 'dielectric', albedo = [0.9, 0.95, 1.0] },
]

planes = [
    { material = 0 }
]

spheres = [
    { material = 1, position = [0.2, 2.6, -0.6], radius = 0.7 },
    { material = 2, position = [-1.5, 0.5, 0.4] },
    { material = 3, position = [1.7, 0.75, -1.2], radius = 0.75 },
    { material = 4, position = [0.3, 0.45, 1.4], radius = 0.45 },
]
"""

OUT = ROOT / "tests" / "golden"
(OUT / "scenes" / "lights.toml").write_text(LIGHTS_TOML)

from oracle import binding as oracle  # noqa: E402
from tests import light_reference as light_ref  # noqa: E402

width, height, spp, bounces, seed = 64, 36, 20, 8, 21
pod = light_ref.lights_scene(spp=spp, bounces=bounces).describe(width, height)
rgba, rgb, stats = light_ref.render(pod, width, height, light_ref.LIGHTS_TABLE, seed=seed)
rgba_sm, rgb_sm, stats_sm = light_ref.render(pod, width, height, light_ref.LIGHTS_TABLE, seed=seed, sm_materials=True)
np.savez_compressed(OUT / "lights_64x36_spp20.npz", width=width, height=height, spp=spp, max_bounces=bounces, seed=seed, emission=light_ref.LIGHTS_TABLE, rgba=rgba, rgb=rgb, segments=stats["segments"], rgba_sm=rgba_sm,
                    rgb_sm=rgb_sm, segments_sm=stats_sm["segments"])
print("lights_64x36_spp20", stats, stats_sm)
for sm, lit in ((False, rgba), (True, rgba_sm)):
    flat, _, _ = oracle.render(pod, width, height, seed=seed, want_rgb=False, sm_materials=sm)
    share = float((lit != flat).mean())
    print(f"pixels that differ from the flag-less frame ({'sm' if sm else 'mg'} table): {100 * share:.1f} percent")
    assert share > 0.05
