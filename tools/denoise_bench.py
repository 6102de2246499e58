#!/usr/bin/env python3
"""What the guide-buffer denoiser costs next to the 16-sample pass it follows, on scenes/basic.toml at 1920x1080:

    python tools/denoise_bench.py [--repeats N] > profiles/r13/denoise_cost.txt

    guide      device time of guide_frame (rt_hip_guide_device)
    filter k   device time of rt_hip_denoise_device with k iterations, k = 0 .. 6, on the frame's real 16-spp mean and guide; iteration i
               (taps 2^i apart) is the difference filter i+1 - filter i of the medians; filter 0 is the pack-only kernel
    pass       device time of one 16-sample pass of the same frame's accumulation (rt_hip_render_progressive, render_ms of the pass's
               stats): the render kernel as it was before the denoiser existed
    drop-in    rt_hip_denoise_progressive's own render_ms (guide + mean + filter with the default parameters): the first call of an
               accumulation, which builds the guide, and later calls, which find it kept

Each case runs in a fresh child process under its own time limit, and the run stops at the first failure.  A child warms up with
`warmup` untimed rounds, then times `repeats` rounds with device events on the launch stream; a line gives the median with the least
and the most.  The cost that matters is (guide + filter at the default parameters) over the pass: the last line states it."""
import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

WIDTH, HEIGHT, SEED = 1920, 1080, 1
CASES = ["guide", "filter", "pass", "drop-in"]


def child(case, repeats, warmup):
    import rt_amd
    from rt_amd import renderer

    pod = rt_amd.Scene.named("basic").set_sampling(16 * (repeats + warmup + 1)).describe(WIDTH, HEIGHT)
    out = {}
    with rt_amd.HipRayTracer(device=0) as tracer:
        if case in ("guide", "filter"):
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

            tracer.upload(pod)
            guide = torch.zeros((HEIGHT, WIDTH, 8), dtype=torch.float32, device="cuda:0")
            tracer.guide_device(WIDTH, HEIGHT, guide.data_ptr(), stream=stream)
            if case == "guide":
                out["guide"] = timed(lambda: tracer.guide_device(WIDTH, HEIGHT, guide.data_ptr(), stream=stream))
            else:
                _, rgb, _, _ = tracer.render_progressive(pod, WIDTH, HEIGHT, seed=SEED, pass_samples=16, want_rgb=True)  # the real 16-spp mean
                image = torch.from_numpy(rgb).to("cuda:0")
                result = torch.zeros_like(image)
                packed = torch.zeros((HEIGHT, WIDTH), dtype=torch.int32, device="cuda:0")
                for k in range(7):
                    p = renderer.denoise_default_params()
                    p.iterations = k
                    out[f"filter {k}"] = timed(lambda: tracer.denoise_device(WIDTH, HEIGHT, image.data_ptr(), guide.data_ptr(), p, result.data_ptr(), packed.data_ptr(), stream=stream))
                out["default iterations"] = [renderer.denoise_default_params().iterations]
        elif case == "pass":
            times = []
            for round_ in range(warmup + repeats):
                _, _, stats, progress = tracer.render_progressive(pod, WIDTH, HEIGHT, seed=SEED, pass_samples=16)
                assert stats["primary_samples"] == WIDTH * HEIGHT * 16
                if round_ >= warmup:
                    times.append(stats["render_ms"])
            out["pass"] = times
            out["kernel"] = [stats["kernel"]]
        else:
            first, later = [], []
            for round_ in range(warmup + repeats):
                tracer.render_progressive(pod, WIDTH, HEIGHT, seed=SEED + round_, pass_samples=16, stats=False)  # (a new seed: a new accumulation, a fresh guide)
                a = tracer.denoise_progressive()[2]
                b = tracer.denoise_progressive()[2]
                if round_ >= warmup:
                    first.append(a), later.append(b)
            out["drop-in, guide built"], out["drop-in, guide kept"] = first, later
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.repeats, args.warmup)
    print(f"# basic.toml {WIDTH}x{HEIGHT} | device ms: median (least .. most) of {args.repeats} rounds after {args.warmup} warm-up rounds")
    medians = {}
    for case in CASES:
        done = subprocess.run([sys.executable, __file__, "--child", case, "--repeats", str(args.repeats), "--warmup", str(args.warmup)], capture_output=True, text=True, timeout=args.timeout)
        if done.returncode != 0:
            print(f"# {case}: exit status {done.returncode}: stopping\n{done.stderr[-2000:]}")
            return 1
        for name, times in json.loads(done.stdout.strip().splitlines()[-1]).items():
            if isinstance(times[0], (int, float)) and name != "default iterations":
                medians[name] = statistics.median(times)
                print(f"{name:22s} | {medians[name]:8.4f} ({min(times):.4f} .. {max(times):.4f})", flush=True)
            else:
                medians[name] = times[0]
                print(f"# {name}: {times[0]}", flush=True)
    for i in range(6):
        print(f"iteration {i} (step {2**i:2d})   | {medians[f'filter {i + 1}'] - medians[f'filter {i}']:8.4f}   (filter {i + 1} - filter {i})")
    k = medians["default iterations"]
    cost = medians["guide"] + medians[f"filter {k}"]
    print(f"guide + filter at the default parameters ({k} iteration{'s' if k != 1 else ''}) = {cost:.4f} ms = {cost / medians['pass']:.3f} of the 16-sample pass ({medians['pass']:.4f} ms) it follows")
    return 0


if __name__ == "__main__":
    sys.exit(main())
