#!/usr/bin/env python3
"""What adaptive sampling (rt_hip_render_adaptive) costs and saves next to the progressive loop of the same pass size
(rt_hip_render_progressive) through the same build.

    python tools/adaptive_bench.py [--repeats N] > profiles/r16/adaptive_bench.jsonl

Case A: scenes/basic.toml at 1920x1080, cap 256, passes of 16, default parameters — the adaptive loop to completion and the progressive
loop.  Case B: the same with min_samples above the cap, so that nothing stops — the price of the adaptive builds and the update kernel.
Each case runs in a fresh child process under its own time limit, with RT_HIP_FLAG_STATS, and the run stops at the first failure.  A
child runs each loop once to warm up (thrown away), then `repeats` times, adaptive and progressive alternating; a loop's figures are
the sum of its passes' `render_ms` (HIP events on the launch stream; the adaptive passes' include the update kernel) and its wall
time; the line gives the medians over the repeats with the least and the most.  One JSON line per case."""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

WIDTH, HEIGHT, CAP, PASS = 1920, 1080, 256, 16
CASES = {"A": None, "B": 1 << 20}  # min_samples (None: the default)


def child(case, repeats, width, height, cap):
    import rt_amd
    from rt_amd import capi, renderer

    pod = rt_amd.Scene.named("basic").set_sampling(cap).describe(width, height)
    params = renderer.adaptive_default_params()
    if CASES[case] is not None:
        params.min_samples = CASES[case]
    flags = capi.RT_HIP_FLAG_STATS
    loops = {"adaptive": [], "progressive": []}
    with rt_amd.HipRayTracer(device=0) as tracer:
        for repeat in range(repeats + 1):
            seed = 1 + repeat  # (a new accumulation every repeat)
            t0, ms, passes = time.perf_counter(), 0.0, 0
            while True:
                _, _, _, stats, info = tracer.render_adaptive(pod, width, height, seed=seed, flags=flags, pass_samples=PASS, params=params, want_counts=False)
                ms, passes = ms + stats["render_ms"], passes + 1
                if info["complete"]:
                    break
            adaptive = {"render_ms": ms, "wall_ms": (time.perf_counter() - t0) * 1e3, "passes": passes, "samples_traced": info["samples_traced"], "kernel": stats["kernel"]}
            t0, ms, passes = time.perf_counter(), 0.0, 0
            while True:
                _, _, stats, progress = tracer.render_progressive(pod, width, height, seed=seed, flags=flags, pass_samples=PASS)
                ms, passes = ms + stats["render_ms"], passes + 1
                if progress["samples_done"] == progress["samples_total"]:
                    break
            progressive = {"render_ms": ms, "wall_ms": (time.perf_counter() - t0) * 1e3, "passes": passes, "samples_traced": width * height * cap, "kernel": stats["kernel"]}
            if repeat:  # (the first round warms everything up)
                loops["adaptive"].append(adaptive)
                loops["progressive"].append(progressive)
    print(json.dumps(loops))


def summary(runs):
    out = {"passes": runs[-1]["passes"], "samples_traced": runs[-1]["samples_traced"], "kernel": runs[-1]["kernel"]}
    for key in ("render_ms", "wall_ms"):
        values = [r[key] for r in runs]
        out[key] = {"median": round(statistics.median(values), 3), "least": round(min(values), 3), "most": round(max(values), 3)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=180)
    ap.add_argument("--size", default=f"{WIDTH}x{HEIGHT}")
    ap.add_argument("--cap", type=int, default=CAP)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    width, height = (int(v) for v in args.size.split("x"))
    if args.child:
        return child(args.child, args.repeats, width, height, args.cap)
    for case in CASES:
        done = subprocess.run([sys.executable, __file__, "--child", case, "--repeats", str(args.repeats), "--size", args.size, "--cap", str(args.cap)], capture_output=True, text=True, timeout=args.timeout)
        if done.returncode != 0:
            print(json.dumps({"case": case, "exit_status": done.returncode, "stderr": done.stderr[-2000:]}))
            return 1
        loops = json.loads(done.stdout.strip().splitlines()[-1])
        print(json.dumps({"case": case, "scene": "basic", "size": args.size, "cap": args.cap, "pass_samples": PASS, "min_samples": CASES[case] or 32, "repeats": args.repeats, "pixels_x_cap": width * height * args.cap,
                          "adaptive": summary(loops["adaptive"]), "progressive": summary(loops["progressive"])}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
