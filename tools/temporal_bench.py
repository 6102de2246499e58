#!/usr/bin/env python3
"""What temporal accumulation costs next to the 16-sample frame it follows, on scenes/basic.toml at 1920x1080:

    python tools/temporal_bench.py [--repeats N] > profiles/r14/temporal_cost.txt

    reproject        device time of reproject_frame (rt_hip_reproject_device) on the frame's real 16-spp mean and guide: without a
                     history, with the history of the same camera, and with the history of a camera a dolly step away
    guide+reproject  ... with guide_frame in front of it on the same stream: what a frame adds before any spatial filter
    frame            device time of the one-shot 16-sample frame (rt_hip_render, render_ms of its stats): the render kernel as it is
                     without temporal accumulation
    drop-in          rt_hip_render_temporal's render_ms (frame + guide + reprojection + pack, and with the default spatial filter), the
                     camera a dolly step further on every call

Each line's case — every combination of kernel and history too — runs in a fresh child process of its own under its own time limit,
and the run stops at the first failure.  A child warms up with `warmup` untimed rounds, then times `repeats` rounds with device events on the launch stream; a line gives the median with the least
and the most.  The cost that matters is (guide + reprojection) over the frame: the last line states it."""
import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

WIDTH, HEIGHT, SEED, SPP = 1920, 1080, 1, 16
HISTORIES = ["no history", "same camera", "a dolly step"]
CASES = [f"{kernel}, {history}" for kernel in ("reproject", "guide+reproject") for history in HISTORIES] + ["frame", "drop-in", "drop-in + default filter"]


def pod_at(step):
    import rt_amd

    return rt_amd.Scene.named("basic").set_camera((0.05 * step, 1.0, 3.0), (0.0, 0.0, -1.0)).set_sampling(SPP).describe(WIDTH, HEIGHT)


def child(case, repeats, warmup):
    import numpy as np

    import rt_amd
    from rt_amd import renderer

    out = {}
    with rt_amd.HipRayTracer(device=0) as tracer:
        if case.partition(", ")[2] in HISTORIES:
            import torch

            stream = torch.cuda.current_stream().cuda_stream

            def timed(launch):
                times = []
                for round_ in range(warmup + repeats):
                    begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    begin.record()
                    launch()
                    end.record()
                    end.synchronize()
                    if round_ >= warmup:
                        times.append(begin.elapsed_time(end))
                return times

            def buffers():
                return (torch.zeros((HEIGHT, WIDTH, 3), dtype=torch.float32, device="cuda:0"), torch.zeros((HEIGHT, WIDTH, 8), dtype=torch.float32, device="cuda:0"))

            found = torch.zeros((1,), dtype=torch.int32, device="cuda:0")
            guide = torch.zeros((HEIGHT, WIDTH, 8), dtype=torch.float32, device="cuda:0")
            histories = {}
            for step in (0, 1):  # the history a first frame leaves under either camera
                pod = pod_at(step)
                image = torch.from_numpy(tracer.render(pod, WIDTH, HEIGHT, seed=SEED + step, want_rgb=True)[1]).to("cuda:0")
                tracer.guide_device(WIDTH, HEIGHT, guide.data_ptr(), stream=stream)
                rgb, record = buffers()
                tracer.reproject_device(WIDTH, HEIGHT, None, guide.data_ptr(), image.data_ptr(), SPP, None, None, None, rgb.data_ptr(), record.data_ptr(), None, stream=stream)
                histories[step] = (np.array(list(pod.inverse_view_projection), dtype=np.float32), rgb, record)
            torch.cuda.synchronize()
            # the current frame is camera 1's (resident since the loop above); `image` and `guide` are its mean and guide
            rgb_out, record_out = buffers()

            def step_with(history, with_guide):
                if with_guide:
                    tracer.guide_device(WIDTH, HEIGHT, guide.data_ptr(), stream=stream)
                matrix, rgb, record = history if history is not None else (None, None, None)
                tracer.reproject_device(WIDTH, HEIGHT, matrix, guide.data_ptr(), image.data_ptr(), SPP, rgb.data_ptr() if rgb is not None else None, record.data_ptr() if record is not None else None, None, rgb_out.data_ptr(),
                                        record_out.data_ptr(), found.data_ptr(), stream=stream)

            with_guide = case.startswith("guide+reproject")
            history = {"no history": None, "same camera": histories[1], "a dolly step": histories[0]}[case.partition(", ")[2]]
            out[case] = timed(lambda: step_with(history, with_guide))
            out[f"pixels with history: {case}"] = [int(found.cpu().numpy().view(np.uint32)[0])]
        elif case == "frame":
            times = []
            for round_ in range(warmup + repeats):
                _, _, stats = tracer.render(pod_at(round_), WIDTH, HEIGHT, seed=SEED + round_)
                assert stats["primary_samples"] == WIDTH * HEIGHT * SPP
                if round_ >= warmup:
                    times.append(stats["render_ms"])
            out["frame"] = times
            out["kernel"] = [stats["kernel"]]
        else:
            spatial = renderer.denoise_default_params() if case == "drop-in + default filter" else None
            times = []
            for round_ in range(warmup + repeats):
                _, _, stats, info = tracer.render_temporal(pod_at(round_), WIDTH, HEIGHT, seed=SEED + round_, filter=spatial)
                if round_ >= warmup:
                    assert info["restarted"] == 0 and info["pixels_with_history"] > 0
                    times.append(stats["render_ms"])
            out[case] = times
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=120)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.repeats, args.warmup)
    print(f"# basic.toml {WIDTH}x{HEIGHT}, {SPP} spp | device ms: median (least .. most) of {args.repeats} rounds after {args.warmup} warm-up rounds")
    medians = {}
    for case in CASES:
        done = subprocess.run([sys.executable, __file__, "--child", case, "--repeats", str(args.repeats), "--warmup", str(args.warmup)], capture_output=True, text=True, timeout=args.timeout)
        if done.returncode != 0:
            print(f"# {case}: exit status {done.returncode}: stopping\n{done.stderr[-2000:]}")
            return 1
        for name, times in json.loads(done.stdout.strip().splitlines()[-1]).items():
            if len(times) > 1:
                medians[name] = statistics.median(times)
                print(f"{name:34s} | {medians[name]:8.4f} ({min(times):.4f} .. {max(times):.4f})", flush=True)
            else:
                print(f"# {name}: {times[0]}", flush=True)
    cost = medians["guide+reproject, a dolly step"]
    print(f"guide + reprojection across a dolly step = {cost:.4f} ms = {cost / medians['frame']:.3f} of the {SPP}-sample frame ({medians['frame']:.4f} ms) they follow")
    print(f"the drop-in's frame = {medians['drop-in']:.4f} ms = {medians['drop-in'] / medians['frame']:.3f} of that frame; with the default spatial filter {medians['drop-in + default filter']:.4f} ms")
    return 0


if __name__ == "__main__":
    sys.exit(main())
