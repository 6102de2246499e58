#!/usr/bin/env python3
"""What the lens builds cost (RT_HIP_FLAG_THIN_LENS): basic.toml at 1920x1080x64,

    (a) flagless        today's frame of the scene: the scalar-register kernel
    (b) no_aperture     the flag with a lens of radius 0: must be the flag-less plan — the same kernel, the same segments
    (c) force_resident  RT_HIP_FLAG_FORCE_RESIDENT, flag-less: the kernel family the lens builds belong to
    (d) lens            the flag with aperture=0.05,focus=4.2: the resident kernel's lens build

The lens' own price is (d) against (c), the price of the kernel family (c) against (a).  (a) and (d) are different frames — the rays
differ — so the line to read next to the milliseconds is ns per segment, and the whole is a record, not a gate.

    python tools/lens_bench.py [--repeats N] > profiles/r33/lens_bench.jsonl

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
CASES = ["flagless", "no_aperture", "force_resident", "lens"]
LENS = (0.05, 4.2)


def child(case, repeats):
    import rt_amd
    from rt_amd import capi

    pod = rt_amd.Scene.named("basic").set_sampling(SPP).describe(WIDTH, HEIGHT)
    flags = {"flagless": 0, "no_aperture": capi.RT_HIP_FLAG_THIN_LENS, "force_resident": capi.RT_HIP_FLAG_FORCE_RESIDENT, "lens": capi.RT_HIP_FLAG_THIN_LENS}[case]
    lens = (0.0, LENS[1]) if case == "no_aperture" else LENS
    times, kernel, segments = [], None, 0
    with rt_amd.HipRayTracer(device=0) as tracer:
        if flags & capi.RT_HIP_FLAG_THIN_LENS:
            tracer.set_lens(*lens)
        for repeat in range(repeats + 1):
            _, _, stats = tracer.render(pod, WIDTH, HEIGHT, seed=1, flags=flags)
            kernel, segments = stats["kernel"], stats["segments"]
            if repeat:  # (the first frame warms everything up)
                times.append(stats["render_ms"])
    median = statistics.median(times)
    print(json.dumps({"case": case, "scene": "basic.toml", "width": WIDTH, "height": HEIGHT, "spp": SPP, "flags": flags, "aperture_radius": lens[0] if flags & capi.RT_HIP_FLAG_THIN_LENS else None, "kernel": kernel,
                      "segments": segments, "repeats": repeats, "render_ms_median": round(median, 4), "render_ms_min": round(min(times), 4), "render_ms_max": round(max(times), 4), "ns_per_segment": round(median * 1e6 / segments, 5)}))


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
