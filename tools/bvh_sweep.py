#!/usr/bin/env python3
"""RT_HIP_FLAG_BVH against the linear kernels, frame by frame, on one GPU (profiles/r06/):

    python tools/bvh_sweep.py [--cases basic,64,1000,...] [--repeats 3] [--out profiles/r06/bvh_sweep.jsonl]
    python tools/bvh_sweep.py --check [--cases 100000]     # the RT_HIP_BVH_CHECK build: every query answered twice

Each case renders the same frame (1920x1080 at BASELINE's sample counts: 256 spp for rt's own scenes, 64 for the sphere
fields) without and with the flag, and prints one JSON line: render_ms (HIP events) and the call's wall time, each the median
over the repeats after one warm-up, the kernel each side ran, and whether the two frames are the same bytes (sha256).
--check runs an experiment library built with -DRT_HIP_BVH_CHECK (make variant NAME=bvhcheck DEFS=-DRT_HIP_BVH_CHECK), whose
BVH kernel also runs the linear scan for every query and counts the answers that differ: the count must be 0."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

DEFAULT_CASES = "basic,dielectric,64,256,1000,1300,3000,10000,30000,100000"


def scene_for(case):
    import rt_amd

    if case in ("basic", "dielectric"):
        return rt_amd.Scene.named(case).set_sampling(256), 256
    return rt_amd.Scene.synthetic(int(case)).set_sampling(64), 64


def run_case(tracer, case, width, height, repeats, seed=1):
    from rt_amd import capi

    scene, spp = scene_for(case)
    pod = scene.describe(width, height)
    line = {"case": case, "spheres": int(pod.n_spheres), "planes": int(pod.n_planes), "width": width, "height": height, "spp": spp}
    digests = {}
    for side, flags in (("linear", 0), ("bvh", capi.RT_HIP_FLAG_BVH)):
        render_ms, call_ms = [], []
        for k in range(repeats + 1):
            t0 = time.perf_counter()
            rgba, _, stats = tracer.render(pod, width, height, seed=seed, flags=flags)
            wall = (time.perf_counter() - t0) * 1e3
            if k:  # (the first call is the warm-up: code objects, the tree's build)
                render_ms.append(stats["render_ms"])
                call_ms.append(wall)
        digests[side] = hashlib.sha256(rgba.tobytes()).hexdigest()
        line[side] = {"kernel": stats["kernel"], "render_ms": round(statistics.median(render_ms), 3), "call_ms": round(statistics.median(call_ms), 3), "segments": int(stats["segments"])}
    line["frame_equal"] = digests["linear"] == digests["bvh"] and line["linear"]["segments"] == line["bvh"]["segments"]
    line["speedup"] = round(line["linear"]["render_ms"] / line["bvh"]["render_ms"], 3) if line["bvh"]["render_ms"] else None
    return line


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", default=DEFAULT_CASES)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--repeats", type=int, default=3, help="timed renders per side after one warm-up (cases above 10 000 spheres: 1)")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    ap.add_argument("--bvh-only", action="store_true", help="render each case once with the flag and nothing else (a profiler's run)")
    ap.add_argument("--check", action="store_true", help="run the RT_HIP_BVH_CHECK experiment library and report its disagreement count")
    args = ap.parse_args()
    if args.check and "RT_HIP_LIBRARY" not in os.environ:
        lib = ROOT / "rt_amd" / "lib" / "librt_hip_bvhcheck.so"
        if not lib.exists():
            subprocess.run(["make", "-C", str(ROOT), "variant", "NAME=bvhcheck", "DEFS=-DRT_HIP_BVH_CHECK", "-j16"], check=True)
        env = dict(os.environ, RT_HIP_LIBRARY=str(lib))
        return subprocess.run([sys.executable, *sys.argv], env=env).returncode

    import rt_amd
    from rt_amd import capi

    out = open(args.out, "a") if args.out else None
    with rt_amd.HipRayTracer(device=0) as tracer:
        for case in args.cases.split(","):
            if args.check or args.bvh_only:
                scene, spp = scene_for(case)
                pod = scene.describe(args.width, args.height)
                _, _, stats = tracer.render(pod, args.width, args.height, seed=1, flags=capi.RT_HIP_FLAG_BVH)  # the library prints bvh_check: ... on stderr
                line = {"case": case, "check": args.check, "kernel": stats["kernel"], "segments": int(stats["segments"]), "render_ms": round(stats["render_ms"], 3)}
            else:
                repeats = args.repeats if case in ("basic", "dielectric") or int(case) <= 10000 else 1
                line = run_case(tracer, case, args.width, args.height, repeats)
            text = json.dumps(line)
            print(text, flush=True)
            if out:
                out.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
