#!/usr/bin/env python3
"""What building the sphere hierarchy costs, host builder (RT_HIP_FLAG_BVH) against device builder
(RT_HIP_FLAG_BVH_DEVICE_BUILD), and what the two trees cost a cached frame.

    python tools/bvh_build_bench.py [--parent-library PATH] [--sizes 1000,10000,...] [--repeats N] > profiles/r09/bvh_device_build.txt

For random fields of each size, each CASE runs in a fresh child process under its own time limit, and the sweep stops at the
first failure.  A case is (library, builder): the head library with both builders and — if --parent-library names the parent
commit's librt_hip.so — the parent's host builder, alternating with the head's.  A child, per repeat (after one warm-up pass of
the whole sequence that is thrown away): moves one sphere and renders a first frame at 480x270x16 spp with stats (`upload_ms`
holds the upload and the build; the upload alone is measured by a linear frame after another move and subtracted), then a cached
frame at 480x270x16 and at 1920x1080x64 (`render_ms`).  Frames are compared with the linear frame's bytes at 480x270.
Figures are medians over the repeats with the least and the most."""
import argparse
import json
import os
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def field(count, seed):
    import numpy as np

    rng = np.random.default_rng(seed)
    side = max(12.0, 12.0 * (count / 2000.0) ** 0.5)  # the same density of spheres at every size
    rows = [(0.0, -1000.0, 0.0, 1000.0, 0)]
    r = rng.uniform(0.05, 0.3, count - 1)
    x, z = rng.uniform(-side, side, count - 1), rng.uniform(-2 * side, 0, count - 1)
    m = rng.integers(1, 5, count - 1)
    rows += list(zip(x.tolist(), r.tolist(), z.tolist(), r.tolist(), m.tolist()))
    return rows


def child(count, builder, repeats):
    import numpy as np

    import rt_amd
    from rt_amd import capi

    materials = [(0, 1, 1, 1, 1, 0.5, 0.5), (1, 0.9, 0.9, 0.9, 1, 0.1, 0.8), (0, 0.3, 0.6, 0.9, 1, 0.5, 0.5), (2, 1, 1, 1, 1, 0.0, 1.5), (1, 0.8, 0.6, 0.2, 1, 0.4, 0.8)]
    flags = capi.RT_HIP_FLAG_BVH | (getattr(capi, "RT_HIP_FLAG_BVH_DEVICE_BUILD", 1 << 11) if builder == "device" else 0)
    rows = field(count, 7)
    camera = rt_amd.Scene.parse("").set_camera((0.0, 4.0, 3.0), (0.0, -0.35, -1.0))

    def pod(width, height, spp, nudge):
        moved = list(rows)
        x, y, z, r, m = moved[1]
        moved[1] = (x + 1e-3 * nudge, y, z, r, m)
        ivp = camera.describe(width, height).inverse_view_projection[:]
        return rt_amd.scene_from_arrays(moved, [], materials, samples_per_pixel=spp, max_bounces=7, inverse_view_projection=ivp)

    out = {"first_upload_ms": [], "upload_alone_ms": [], "render_small_ms": [], "render_large_ms": [], "equal": True}
    with rt_amd.HipRayTracer(device=0) as tracer:
        nudge = 0
        for repeat in range(repeats + 1):
            nudge += 1
            rgba, _, stats = tracer.render(pod(480, 270, 16, nudge), 480, 270, seed=1, flags=flags)
            _, _, small = tracer.render(pod(480, 270, 16, nudge), 480, 270, seed=1, flags=flags)
            _, _, large = tracer.render(pod(1920, 1080, 64, nudge), 1920, 1080, seed=1, flags=flags)
            if repeat == 0 and count <= 100000:  # the linear frame of the large scenes takes seconds: compared at the sizes that do not
                want, _, _ = tracer.render(pod(480, 270, 16, nudge), 480, 270, seed=1)
                out["equal"] = bool(np.array_equal(rgba, want))
            nudge += 1
            tracer.upload(pod(480, 270, 16, nudge))
            alone = tracer.stats()["upload_ms"]
            if repeat:  # (the first pass warms everything up)
                out["first_upload_ms"].append(stats["upload_ms"])
                out["upload_alone_ms"].append(alone)
                out["render_small_ms"].append(small["render_ms"])
                out["render_large_ms"].append(large["render_ms"])
    print(json.dumps(out))


def spread(values):
    return f"{statistics.median(values):10.3f} ({min(values):.3f} .. {max(values):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-library", default=None)
    ap.add_argument("--sizes", default="1000,10000,100000,1000000")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--child", nargs=2, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(int(args.child[0]), args.child[1], args.repeats)
    cases = [("head", "host", None), ("head", "device", None)]
    if args.parent_library:
        cases = [("parent", "host", args.parent_library), ("head", "host", None), ("parent", "host", args.parent_library), ("head", "host", None), ("head", "device", None)]
    print("# spheres library builder | first frame upload_ms | upload alone ms | build ms (difference of medians) | cached 480x270x16 render_ms | cached 1920x1080x64 render_ms | equal")
    for count in (int(v) for v in args.sizes.split(",")):
        for library, builder, path in cases:
            env = dict(os.environ)
            env.pop("RT_HIP_LIBRARY", None)
            if path:
                env["RT_HIP_LIBRARY"] = path
            done = subprocess.run([sys.executable, __file__, "--child", str(count), builder, "--repeats", str(args.repeats)], env=env, capture_output=True, text=True, timeout=args.timeout)
            if done.returncode != 0:
                print(f"# {count} {library} {builder}: exit status {done.returncode}: stopping\n{done.stderr[-2000:]}")
                return 1
            r = json.loads(done.stdout.strip().splitlines()[-1])
            build = statistics.median(r["first_upload_ms"]) - statistics.median(r["upload_alone_ms"])
            print(f"{count:8d} {library:6s} {builder:6s} | {spread(r['first_upload_ms'])} | {spread(r['upload_alone_ms'])} | {build:10.3f} | {spread(r['render_small_ms'])} | {spread(r['render_large_ms'])} | {r['equal']}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
