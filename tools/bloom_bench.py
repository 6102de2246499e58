#!/usr/bin/env python3
"""What bloom costs, at 1920x1080:

    python tools/bloom_bench.py [--repeats N] > profiles/r30/bloom_bench.jsonl

One JSON line per case:
    bloom:levels=1    rt_hip_bloom_device (frame and layer out) on a positive noise frame, a tenth of its pixels above the threshold,
    bloom:levels=6    with that many levels asked for: device events around the call, which is 2 x levels launches
    bloom:levels=8    (prefilter, levels - 1 down, levels - 1 up, composite) and nothing else
    bloom:in-place    six levels, the frame in place and no layer: what rt_hip_render_bloomed enqueues
    tonemap           rt_hip_tonemap_device of the same build on the same frame (histogram, exposure, pixels), to set the figures beside

Each case runs in a fresh child process under its own time limit, and the run stops at the first failure.  A child warms up with
`warmup` untimed rounds, then times `repeats` rounds; a line gives the median with the least and the most, in milliseconds of device
time, and the bytes the launches move by the level plan.  A record: nothing in the header or in DESIGN.md promises a speed."""
import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

WIDTH, HEIGHT = 1920, 1080
CASES = ["bloom:levels=1", "bloom:levels=6", "bloom:levels=8", "bloom:in-place", "tonemap"]


def noise():
    import numpy as np

    rng = np.random.default_rng(1)
    rgb = rng.uniform(0.01, 0.9, size=(HEIGHT, WIDTH, 3))
    bright = rng.random((HEIGHT, WIDTH)) < 0.1
    rgb[bright] *= np.exp2(rng.uniform(1.0, 6.0, size=(int(bright.sum()), 1))) / 0.45
    return rgb.astype(np.float32)


def bytes_moved(levels, frame_out, layer_out):
    """By the plan: every launch reads its source once and writes its destination once (bloom_down's 35 x 35 tiles re-read their rims:
    not counted)."""
    sizes, w, h = [], WIDTH, HEIGHT
    while len(sizes) < levels:
        w, h = -(-w // 2), -(-h // 2)
        sizes.append(w * h * 12)
        if (w, h) == (1, 1):
            break
    full = WIDTH * HEIGHT * 12
    prefilter = full + sizes[0]
    down = sum(a + b for a, b in zip(sizes, sizes[1:]))
    up = sum(b + 2 * a for a, b in zip(sizes, sizes[1:]))
    composite = sizes[0] + (2 * full if frame_out else 0) + (full if layer_out else 0)
    return prefilter + down + up + composite, len(sizes)


def child(case, repeats, warmup):
    import torch

    import rt_amd
    from rt_amd import renderer

    out = {"case": case, "width": WIDTH, "height": HEIGHT}
    with rt_amd.HipRayTracer(device=0) as tracer:
        stream = torch.cuda.current_stream().cuda_stream
        frame = torch.from_numpy(noise()).to("cuda:0")
        rgb = torch.zeros((HEIGHT, WIDTH, 3), dtype=torch.float32, device="cuda:0")
        if case == "tonemap":
            state = torch.zeros((8,), dtype=torch.int32, device="cuda:0")
            rgba = torch.zeros((HEIGHT, WIDTH), dtype=torch.int32, device="cuda:0")
            call = lambda: tracer.tonemap_device(WIDTH, HEIGHT, frame.data_ptr(), state.data_ptr(), None, rgb.data_ptr(), rgba.data_ptr(), stream=stream)
            out.update(launches=3, bytes_moved=WIDTH * HEIGHT * (12 + 12 + 12 + 4))
        else:
            params = renderer.bloom_default_params()
            in_place = case == "bloom:in-place"
            if not in_place:
                params.levels = int(case.split("=")[1])
            layer = None if in_place else torch.zeros((HEIGHT, WIDTH, 3), dtype=torch.float32, device="cuda:0")
            call = lambda: tracer.bloom_device(WIDTH, HEIGHT, frame.data_ptr(), params, frame.data_ptr() if in_place else rgb.data_ptr(), None if in_place else layer.data_ptr(), stream=stream)
            moved, levels = bytes_moved(params.levels, True, not in_place)
            out.update(launches=2 * levels, bytes_moved=moved, **renderer.bloom_plan(WIDTH, HEIGHT, params))
            assert out["levels"] == levels
        times = []
        for round_ in range(warmup + repeats):
            begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            begin.record()
            call()
            end.record()
            end.synchronize()
            if round_ >= warmup:
                times.append(begin.elapsed_time(end))
    out.update(ms_median=statistics.median(times), ms_min=min(times), ms_max=max(times), repeats=repeats, warmup=warmup)
    out["gb_per_s_at_median"] = out["bytes_moved"] / out["ms_median"] / 1e6
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=120)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.repeats, args.warmup)
    for case in CASES:
        done = subprocess.run([sys.executable, __file__, "--child", case, "--repeats", str(args.repeats), "--warmup", str(args.warmup)], capture_output=True, text=True, timeout=args.timeout)
        if done.returncode != 0:
            print(json.dumps({"case": case, "exit_status": done.returncode, "stderr": done.stderr[-2000:]}), flush=True)
            return 1
        print(done.stdout.strip().splitlines()[-1], flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
