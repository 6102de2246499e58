#!/usr/bin/env python3
"""Which contract branches do the frames the GPU suite ALREADY renders reach?  The oracle's branch census (oracle_render_census) over
    - CASES of tests/test_gpu_parity.py (test_frame_is_bit_exact), mg table,
    - the 24 random scenes of test_random_scenes_are_bit_exact, under both scatter tables,
    - the committed golden frames (tests/golden/*_spp*.npz), mg table,
written as a table: event x how many of those frames reach it at least once, and the total count.  CPU only; a few minutes, most of it
the two big synthetic frames.  tests/test_rare_branches.py reads the table: every event must be reached by a frame of this table or by
a constructed case of tests/rare_cases.py.

    python tools/branch_census.py > profiles/r18/branch_census.txt"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import rt_amd  # noqa: E402
from oracle import binding as oracle  # noqa: E402
from tests import test_gpu_parity as parity  # noqa: E402
from tests.conftest import GOLDEN, PLANES_SCENE  # noqa: E402


def frames():
    """(label, pod, width, height, seed, sm table) of every frame."""
    for name, width, height, spp, bounces, seed in parity.CASES:
        scene = rt_amd.Scene.parse(PLANES_SCENE) if name == "planes" else rt_amd.Scene.named(name)
        yield f"CASES {name} {width}x{height}x{spp}", scene.set_sampling(spp, bounces).describe(width, height), width, height, seed, False
    for case in range(24):
        rng = np.random.default_rng(1000 + case)  # (the lines of test_random_scenes_are_bit_exact)
        spheres, planes, materials, camera = parity.random_scene(rng)
        width, height = int(rng.integers(17, 140)), int(rng.integers(9, 90))
        spp, bounces = int(rng.integers(1, 40)), int(rng.integers(1, 12))
        if case % 4 == 3:
            spp = int(rng.integers(40, 140))
        ivp = camera.describe(width, height).inverse_view_projection[:]
        pod = rt_amd.scene_from_arrays(spheres, planes, materials, samples_per_pixel=spp, max_bounces=bounces, inverse_view_projection=ivp)
        seed = int(rng.integers(0, 2**63))
        for sm in (False, True):
            yield f"random scene {case} {'sm' if sm else 'mg'}", pod, width, height, seed, sm
    for fixture in ("basic_64x36_spp4", "dielectric_64x36_spp4", "planes_48x27_spp4", "synthetic1500_32x18_spp2"):
        golden = np.load(GOLDEN / f"{fixture}.npz")
        name = str(golden["scene"])
        scene = rt_amd.Scene.parse(PLANES_SCENE) if name == "planes" else rt_amd.Scene.named(name)
        width, height = int(golden["width"]), int(golden["height"])
        yield f"golden {fixture}", scene.set_sampling(int(golden["spp"]), int(golden["max_bounces"])).describe(width, height), width, height, int(golden["seed"]), False


def main():
    reached = dict.fromkeys(oracle.CENSUS_EVENTS, 0)
    total = dict.fromkeys(oracle.CENSUS_EVENTS, 0)
    n = 0
    for label, pod, width, height, seed, sm in frames():
        counts = oracle.render_census(pod, width, height, seed=seed, sm_materials=sm)[3]
        n += 1
        for event, count in counts.items():
            reached[event] += count > 0
            total[event] += count
        print(label, {e: c for e, c in counts.items() if c}, file=sys.stderr)
    print(f"# the oracle's branch census over the {n} frames the GPU parity suite renders (tools/branch_census.py):")
    print("# event, frames that reach it, occurrences in all frames together")
    for event in oracle.CENSUS_EVENTS:
        print(f"{event:28s} {reached[event]:4d} {total[event]:14d}")


if __name__ == "__main__":
    main()
