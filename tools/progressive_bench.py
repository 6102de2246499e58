#!/usr/bin/env python3
"""What a frame costs in passes (rt_hip_render_progressive) next to the same frame in one launch through the SAME kernel family of
the same build — per pass the progressive frame pays a launch, 12 bytes per pixel of accumulator read and written, and the
per-pixel finish (division, square roots, pack, store).

    python tools/progressive_bench.py [--repeats N] > profiles/r11/progressive_cost.txt

Cases: scenes/basic.toml at 1920x1080x256 — one shot with RT_HIP_FLAG_FORCE_RESIDENT, passes of 16, passes of 64 — and a field of
10 000 spheres at 1920x1080x64 with RT_HIP_FLAG_BVH — one shot, passes of 16.  Each case runs in a fresh child process under its own
time limit, and the run stops at the first failure.  A child renders the frame once to warm up (thrown away), then `repeats` times;
a frame's figure is the sum of its launches' `render_ms` (HIP events on the launch stream), and the line gives the median over the
repeats with the least and the most.  The last frame's bytes are compared with the one-shot frame's."""
import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

WIDTH, HEIGHT = 1920, 1080
CASES = [  # (scene, samples per pixel, pass_samples: 0 = one shot)
    ("basic", 256, 0),
    ("basic", 256, 16),
    ("basic", 256, 64),
    ("field10000", 64, 0),
    ("field10000", 64, 16),
]


def child(scene, spp, pass_samples, repeats):
    import hashlib

    import numpy as np

    import rt_amd
    from rt_amd import capi
    from tools.bvh_build_bench import field

    if scene == "basic":
        pod = rt_amd.Scene.named("basic").set_sampling(spp).describe(WIDTH, HEIGHT)
        pass_flags, one_shot_flags = 0, capi.RT_HIP_FLAG_FORCE_RESIDENT
    else:
        materials = [(0, 1, 1, 1, 1, 0.5, 0.5), (1, 0.9, 0.9, 0.9, 1, 0.1, 0.8), (0, 0.3, 0.6, 0.9, 1, 0.5, 0.5), (2, 1, 1, 1, 1, 0.0, 1.5), (1, 0.8, 0.6, 0.2, 1, 0.4, 0.8)]
        ivp = rt_amd.Scene.parse("").set_camera((0.0, 4.0, 3.0), (0.0, -0.35, -1.0)).describe(WIDTH, HEIGHT).inverse_view_projection[:]
        pod = rt_amd.scene_from_arrays(field(10000, 7), [], materials, samples_per_pixel=spp, max_bounces=7, inverse_view_projection=ivp)
        pass_flags = one_shot_flags = capi.RT_HIP_FLAG_BVH
    frames, kernels, launches = [], set(), 0
    with rt_amd.HipRayTracer(device=0) as tracer:
        for repeat in range(repeats + 1):
            total, launches = 0.0, 0
            if pass_samples == 0:
                rgba, _, stats = tracer.render(pod, WIDTH, HEIGHT, seed=1, flags=one_shot_flags)
                total, launches = stats["render_ms"], 1
                kernels.add(stats["kernel"])
            else:
                seed = 1 + repeat  # (a new accumulation every repeat; the last one's seed is the compared frame's)
                while True:
                    rgba, _, stats, progress = tracer.render_progressive(pod, WIDTH, HEIGHT, seed=seed, flags=pass_flags, pass_samples=pass_samples)
                    total, launches = total + stats["render_ms"], launches + 1
                    kernels.add(stats["kernel"])
                    if progress["samples_done"] == progress["samples_total"]:
                        break
            if repeat:  # (the first frame warms everything up)
                frames.append(total)
        want, _, _ = tracer.render(pod, WIDTH, HEIGHT, seed=1 if pass_samples == 0 else repeats + 1, flags=one_shot_flags)
    print(json.dumps({"frame_ms": frames, "launches": launches, "kernels": sorted(kernels), "equal": bool(np.array_equal(rgba, want)), "sha256": hashlib.sha256(np.ascontiguousarray(want).tobytes()).hexdigest()[:16]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=120)
    ap.add_argument("--child", nargs=3, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child[0], int(args.child[1]), int(args.child[2]), args.repeats)
    print(f"# scene spp pass_samples (0 = one shot) | launches per frame | sum of the launches' render_ms: median (least .. most) of {args.repeats} frames | kernel | last frame equals the one-shot frame")
    for scene, spp, pass_samples in CASES:
        done = subprocess.run([sys.executable, __file__, "--child", scene, str(spp), str(pass_samples), "--repeats", str(args.repeats)], capture_output=True, text=True, timeout=args.timeout)
        if done.returncode != 0:
            print(f"# {scene} {spp} {pass_samples}: exit status {done.returncode}: stopping\n{done.stderr[-2000:]}")
            return 1
        r = json.loads(done.stdout.strip().splitlines()[-1])
        print(f"{scene:11s} {spp:4d} {pass_samples:3d} | {r['launches']:3d} | {statistics.median(r['frame_ms']):9.3f} ({min(r['frame_ms']):.3f} .. {max(r['frame_ms']):.3f}) | {','.join(r['kernels'])} | {r['equal']}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
