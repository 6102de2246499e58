#!/usr/bin/env python3
"""RT_HIP_FLAG_BOX_BVH against the linear box builds, and beyond their 256 boxes, on one GPU (profiles/r15/):

    python tools/box_bvh_bench.py [--cases 64,256,1000,10000,100000] [--repeats 5] [--out profiles/r15/box_bvh_sweep.jsonl]

Each case is a square grid of boxes over a ground plane at 1920x1080x64, rendered in a fresh child process of its own under its own
time limit; the first failure stops the run.  Up to 256 boxes the same frame is rendered with RT_HIP_FLAG_TRACE_BOXES alone (the
linear scan from LDS) and with RT_HIP_FLAG_BOX_BVH, and the two frames are compared for equality; beyond, through the tree only.  One
JSON line per case: per side the kernel, render_ms (HIP events; the median of the repeats after the first frame, least .. most) and
the FIRST frame's upload_ms — the scene's upload and, with the flag, the host build of the tree."""
import argparse
import hashlib
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

DEFAULT_CASES = "64,256,1000,10000,100000"
LINEAR_MAX_BOXES = 256


def grid_scene(count, width, height, spp):
    """`count` boxes on a square grid of pitch 0.5 around the camera's line of sight, heights from a small hash, four materials."""
    import numpy as np

    import rt_amd
    from rt_amd.scene import scene_from_arrays

    side = int(np.ceil(np.sqrt(count)))
    pitch = 12.0 / side  # the field keeps its footprint: more boxes are smaller boxes
    i = np.arange(count)
    height_of = 0.1 * pitch + 0.9 * pitch * (((i * 2654435761) >> 7) % 97) / 96.0
    boxes = np.stack([(i % side - side / 2 + 0.5) * pitch, height_of, 2.0 - (i // side) * pitch, np.full(count, 0.35 * pitch), height_of, np.full(count, 0.35 * pitch), i % 4], axis=1)
    camera = rt_amd.Scene.named("basic").set_camera((0.0, 3.0, 6.0), (0.0, -0.45, -1.0)).describe(width, height)
    materials = [(0, 0.8, 0.8, 0.3, 1.0, 0.0, 1.0), (1, 0.9, 0.6, 0.4, 1.0, 0.2, 0.9), (0, 0.3, 0.5, 0.8, 1.0, 0.0, 0.8), (0, 0.7, 0.3, 0.3, 1.0, 0.0, 0.9)]
    return scene_from_arrays(spheres=None, planes=[(0, 1, 0, 0, 0)], materials=materials, boxes=boxes, samples_per_pixel=spp, max_bounces=8,
                             inverse_view_projection=np.array(list(camera.inverse_view_projection), dtype=np.float32).reshape(4, 4))


def child(count, width, height, spp, repeats):
    import rt_amd
    from rt_amd import capi

    pod = grid_scene(count, width, height, spp)
    line = {"boxes": count, "width": width, "height": height, "spp": spp, "repeats": repeats}
    sides = [("tree", capi.RT_HIP_FLAG_TRACE_BOXES | capi.RT_HIP_FLAG_BOX_BVH)]
    if count <= LINEAR_MAX_BOXES:
        sides.insert(0, ("linear", capi.RT_HIP_FLAG_TRACE_BOXES))
    digests = {}
    for side, flags in sides:
        with rt_amd.HipRayTracer(device=0) as tracer:  # (a context of its own: the first frame uploads the scene and builds the tree)
            times, first_upload = [], None
            for k in range(repeats + 1):
                rgba, _, stats = tracer.render(pod, width, height, seed=1, flags=flags)
                if k == 0:
                    first_upload = stats["upload_ms"]
                else:
                    times.append(stats["render_ms"])
            digests[side] = (hashlib.sha256(rgba.tobytes()).hexdigest(), int(stats["segments"]))
            line[side] = {"kernel": stats["kernel"], "render_ms": round(statistics.median(times), 3), "least": round(min(times), 3), "most": round(max(times), 3), "first_upload_ms": round(first_upload, 3), "segments": int(stats["segments"])}
    if "linear" in line:
        line["frame_equal"] = digests["linear"] == digests["tree"]
        line["tree_over_linear"] = round(line["tree"]["render_ms"] / line["linear"]["render_ms"], 3)
    print(json.dumps(line), flush=True)
    return 0 if line.get("frame_equal", True) else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", default=DEFAULT_CASES)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5, help="timed frames per side after the first")
    ap.add_argument("--timeout", type=int, default=150, help="seconds a case may take")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        return child(args.child, args.width, args.height, args.spp, args.repeats)
    for case in args.cases.split(","):
        command = [sys.executable, str(Path(__file__).resolve()), "--child", case, "--width", str(args.width), "--height", str(args.height), "--spp", str(args.spp), "--repeats", str(args.repeats)]
        try:
            done = subprocess.run(command, capture_output=True, text=True, timeout=args.timeout)
        except subprocess.TimeoutExpired:
            print(f"box_bvh_bench: {case} boxes did not finish within {args.timeout} s; stopping", file=sys.stderr)
            return 1
        sys.stdout.write(done.stdout)
        sys.stdout.flush()
        if done.returncode != 0:
            sys.stderr.write(done.stderr)
            print(f"box_bvh_bench: {case} boxes failed with status {done.returncode}; stopping", file=sys.stderr)
            return 1
        if args.out:
            with open(args.out, "a") as out:
                out.write(done.stdout)
    return 0


if __name__ == "__main__":
    sys.exit(main())
