#!/usr/bin/env python3
"""What an upscaled frame costs next to the whole frame it stands in for, on scenes/basic.toml at 1920x1080:

    python tools/upscale_bench.py [--repeats N] > profiles/r24/upscale_bench.jsonl

One JSON line per case:
    whole           rt_hip_render at 16 spp: render_ms of its stats (the kernel as it was before the upsampler existed)
    upscaled        rt_hip_render_upscaled at factors 2, 3 and 4, each at the SAME spp (16: 1 / factor^2 of the rays) and at
                    factor^2 x the spp (64, 144, 256: the whole frame's ray budget spent on fewer pixels): render_ms of its stats — the
                    traced low frame, both guides and the reconstruction — and the orphans
    upsample_frame  the reconstruction alone (rt_hip_upsample_device on the frame's real low mean and guides, float and packed output
                    and the orphan word), device events around the launch

Each case runs in a fresh child process under its own time limit, and the run stops at the first failure.  A child warms up with
`warmup` untimed rounds, then times `repeats` rounds; a line gives the median with the least and the most, in milliseconds of device
time.  A record: nothing in the header or in DESIGN.md promises a speed."""
import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

WIDTH, HEIGHT, SEED, SPP = 1920, 1080, 1, 16
CASES = ["whole"] + [f"upscaled:{factor}:{spp}" for factor in (2, 3, 4) for spp in (SPP, SPP * factor * factor)] + [f"upsample_frame:{factor}" for factor in (2, 3, 4)]


def child(case, repeats, warmup):
    import rt_amd
    from rt_amd import renderer

    kind, *rest = case.split(":")
    out = {"case": case, "width": WIDTH, "height": HEIGHT}
    with rt_amd.HipRayTracer(device=0) as tracer:
        if kind == "whole":
            pod = rt_amd.Scene.named("basic").set_sampling(SPP).describe(WIDTH, HEIGHT)
            times = []
            for round_ in range(warmup + repeats):
                _, _, stats = tracer.render(pod, WIDTH, HEIGHT, seed=SEED + round_)
                if round_ >= warmup:
                    times.append(stats["render_ms"])
            out.update(spp=SPP, primary_samples=stats["primary_samples"], kernel=stats["kernel"])
        elif kind == "upscaled":
            factor, spp = int(rest[0]), int(rest[1])
            pod = rt_amd.Scene.named("basic").set_sampling(spp).describe(WIDTH, HEIGHT)
            times = []
            for round_ in range(warmup + repeats):
                _, _, stats, info = tracer.render_upscaled(pod, WIDTH, HEIGHT, seed=SEED + round_, factor=factor)
                if round_ >= warmup:
                    times.append(stats["render_ms"])
            out.update(factor=factor, spp=spp, primary_samples=stats["primary_samples"], kernel=stats["kernel"], **info)
        else:
            import torch

            factor = int(rest[0])
            w, h = renderer.upsample_low_size(WIDTH, HEIGHT, factor)
            stream = torch.cuda.current_stream().cuda_stream
            tracer.upload(rt_amd.Scene.named("basic").set_sampling(SPP).describe(WIDTH, HEIGHT))
            low_rgba = torch.zeros((h, w), dtype=torch.int32, device="cuda:0")
            low = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0")
            guide_low = torch.zeros((h, w, 8), dtype=torch.float32, device="cuda:0")
            guide_full = torch.zeros((HEIGHT, WIDTH, 8), dtype=torch.float32, device="cuda:0")
            tracer.render_device(w, h, low_rgba.data_ptr(), seed=SEED, d_rgb_f32=low.data_ptr(), stream=stream)
            tracer.guide_device(w, h, guide_low.data_ptr(), stream=stream)
            tracer.guide_device(WIDTH, HEIGHT, guide_full.data_ptr(), stream=stream)
            rgb = torch.zeros((HEIGHT, WIDTH, 3), dtype=torch.float32, device="cuda:0")
            rgba = torch.zeros((HEIGHT, WIDTH), dtype=torch.int32, device="cuda:0")
            orphans = torch.zeros((1,), dtype=torch.int32, device="cuda:0")
            times = []
            for round_ in range(warmup + repeats):
                begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                begin.record()
                tracer.upsample_device(WIDTH, HEIGHT, w, h, low.data_ptr(), guide_low.data_ptr(), guide_full.data_ptr(), None, rgb.data_ptr(), rgba.data_ptr(), orphans.data_ptr(), stream=stream)
                end.record()
                end.synchronize()
                if round_ >= warmup:
                    times.append(begin.elapsed_time(end))
            moved = WIDTH * HEIGHT * 48 + w * h * 44 + 4
            out.update(factor=factor, low_width=w, low_height=h, orphans=int(orphans.cpu()[0]), bytes_moved=moved, note="events around a memset of one word and the kernel")
    out.update(ms_median=statistics.median(times), ms_min=min(times), ms_max=max(times), repeats=repeats, warmup=warmup)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
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
