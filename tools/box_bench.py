#!/usr/bin/env python3
"""What tracing the boxes costs (RT_HIP_FLAG_TRACE_BOXES): tests/golden/scenes/boxes.toml at 1920x1080x64,

    (a) boxes            with the flag: the resident kernel's box build
    (b) flagless         today's frame of the same scene, boxes not hit: the scalar-register kernel
    (c) flagless_resident the same under RT_HIP_FLAG_FORCE_RESIDENT: the kernel family the box build derives from

so that (a) - (c) is what the boxes cost (their scan, and the paths that now end on them) and (b) what the scene's owner sees today.

    python tools/box_bench.py [--repeats N] > profiles/r12/box_bench.jsonl

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
CASES = ["boxes", "flagless", "flagless_resident"]


def child(case, repeats):
    import rt_amd
    from rt_amd import capi

    flags = {"boxes": capi.RT_HIP_FLAG_TRACE_BOXES, "flagless": 0, "flagless_resident": capi.RT_HIP_FLAG_FORCE_RESIDENT}[case]
    pod = rt_amd.Scene.load(ROOT / "tests" / "golden" / "scenes" / "boxes.toml").set_sampling(SPP).describe(WIDTH, HEIGHT)
    times, kernel, segments = [], None, 0
    with rt_amd.HipRayTracer(device=0) as tracer:
        for repeat in range(repeats + 1):
            _, _, stats = tracer.render(pod, WIDTH, HEIGHT, seed=1, flags=flags)
            kernel, segments = stats["kernel"], stats["segments"]
            if repeat:  # (the first frame warms everything up)
                times.append(stats["render_ms"])
    print(json.dumps({"case": case, "scene": "boxes.toml", "width": WIDTH, "height": HEIGHT, "spp": SPP, "flags": flags, "kernel": kernel, "segments": segments, "repeats": repeats,
                      "render_ms_median": round(statistics.median(times), 4), "render_ms_min": round(min(times), 4), "render_ms_max": round(max(times), 4)}))


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
