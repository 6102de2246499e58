#!/usr/bin/env python3
"""What direct light sampling costs (RT_HIP_FLAG_DIRECT_LIGHT): tests/golden/scenes/lights.toml at 1920x1080x64 under the
fixture's table (lamp=4,3.2,2),

    (a) emission    RT_HIP_FLAG_EMISSION alone: the resident kernel's light build
    (b) direct      ... with RT_HIP_FLAG_DIRECT_LIGHT: its direct build — every lambert vertex adds a shadow segment

The two are different frames with different segment counts — a shadow query is a segment — so the lines to read are the kernel's time,
the segments and ps per segment, and the whole is a record, not a gate: the flag promises nothing about speed.

    python tools/direct_light_bench.py [--repeats N] > profiles/r23/direct_light_bench.jsonl

One JSON line per case.  Each case runs in a fresh child process under its own time limit, and the run stops at the first failure.
A child renders the frame once to warm up (thrown away), then `repeats` times; `render_ms` is the kernel's device time (HIP events on
the launch stream): the median over the repeats, with the least and the most."""
import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

WIDTH, HEIGHT, SPP = 1920, 1080, 64
CASES = ["emission", "direct"]
LAMP = {1: (4.0, 3.2, 2.0)}  # material 1 of lights.toml, "lamp"


def child(case, repeats):
    import numpy as np

    import rt_amd
    from rt_amd import capi

    pod = rt_amd.Scene.load(ROOT / "tests" / "golden" / "scenes" / "lights.toml").set_sampling(SPP).describe(WIDTH, HEIGHT)
    flags = capi.RT_HIP_FLAG_EMISSION | (capi.RT_HIP_FLAG_DIRECT_LIGHT if case == "direct" else 0)
    table = np.zeros((pod.n_materials, 3), dtype=np.float32)
    for material, rgb in LAMP.items():
        table[material] = rgb
    times, kernel, segments = [], None, 0
    with rt_amd.HipRayTracer(device=0) as tracer:
        tracer.set_emission(table)
        for repeat in range(repeats + 1):
            _, _, stats = tracer.render(pod, WIDTH, HEIGHT, seed=1, flags=flags)
            kernel, segments = stats["kernel"], stats["segments"]
            if repeat:  # (the first frame warms everything up)
                times.append(stats["render_ms"])
    median = statistics.median(times)
    print(json.dumps({"case": case, "scene": "lights.toml", "width": WIDTH, "height": HEIGHT, "spp": SPP, "flags": flags, "lights": int((table > 0).any(axis=1).sum()), "kernel": kernel, "segments": segments,
                      "repeats": repeats, "render_ms_median": round(median, 4), "render_ms_min": round(min(times), 4), "render_ms_max": round(max(times), 4), "ps_per_segment": round(median * 1e9 / segments, 2)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--timeout", type=int, default=120)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.repeats)
    for case in CASES:
        done = subprocess.run([sys.executable, __file__, "--child", case, "--repeats", str(args.repeats)], capture_output=True, text=True, timeout=args.timeout)
        if done.returncode != 0:
            print(json.dumps({"case": case, "exit_status": done.returncode, "stderr": done.stderr[-1000:]}), flush=True)
            return 1
        print(done.stdout.strip().splitlines()[-1], flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
