#!/usr/bin/env python3
"""What tone mapping costs, at 1920x1080:

    python tools/tonemap_bench.py [--repeats N] > profiles/r28/tonemap_bench.jsonl

One JSON line per case:
    device:noise    rt_hip_tonemap_device (histogram, exposure, pixels: float and packed output) on channels 2^u, u uniform in [-8, 8):
                    the lanes of a wave scatter over the bins.  Device events around the call: a memset of 257 words and three launches
    device:flat     the same on a frame of ONE colour: all 64 lanes of every wave add to the same LDS word
    device:lights   the same on the traced float mean of tests/golden/scenes/lights.toml (lamp=4,3.2,2, 16 spp)
    device:manual   a manual exposure on the noise frame: two fills and the pixel kernel alone
    render          rt_hip_render of the lights scene at 16 spp with RT_HIP_FLAG_EMISSION: render_ms of its stats
    tonemapped      rt_hip_render_tonemapped of the same frames: render_ms of its stats, the traced frame through the last launch

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
LIGHTS = "lamp=4,3.2,2"
CASES = ["device:noise", "device:flat", "device:lights", "device:manual", "render", "tonemapped"]


def lights_scene(tracer):
    import rt_amd
    from rt_amd import renderer

    scene = rt_amd.Scene.load(ROOT / "tests" / "golden" / "scenes" / "lights.toml").set_sampling(SPP)
    names = ["ground", "lamp", "clay", "brass", "glass"]  # (the scene file's material names, in its order)
    tracer.set_emission(renderer.lights_from_spec(LIGHTS, names))
    return scene.describe(WIDTH, HEIGHT)


def child(case, repeats, warmup):
    import numpy as np

    import rt_amd
    from rt_amd import capi, renderer

    kind, *rest = case.split(":")
    out = {"case": case, "width": WIDTH, "height": HEIGHT}
    with rt_amd.HipRayTracer(device=0) as tracer:
        if kind == "device":
            import torch

            stream = torch.cuda.current_stream().cuda_stream
            if rest[0] == "lights":
                tracer.upload(lights_scene(tracer))
                packed = torch.zeros((HEIGHT, WIDTH), dtype=torch.int32, device="cuda:0")
                frame = torch.zeros((HEIGHT, WIDTH, 3), dtype=torch.float32, device="cuda:0")
                tracer.render_device(WIDTH, HEIGHT, packed.data_ptr(), seed=SEED, flags=capi.RT_HIP_FLAG_EMISSION, d_rgb_f32=frame.data_ptr(), stream=stream)
            elif rest[0] == "flat":
                frame = torch.full((HEIGHT, WIDTH, 3), 0.5, dtype=torch.float32, device="cuda:0")
            else:
                rng = np.random.default_rng(1)
                frame = torch.from_numpy(np.exp2(rng.uniform(-8.0, 8.0, size=(HEIGHT, WIDTH, 3))).astype(np.float32)).to("cuda:0")
            params = renderer.tonemap_default_params()
            if rest[0] == "manual":
                params.exposure = 0.5
            state = torch.zeros((8,), dtype=torch.int32, device="cuda:0")
            rgb = torch.zeros((HEIGHT, WIDTH, 3), dtype=torch.float32, device="cuda:0")
            rgba = torch.zeros((HEIGHT, WIDTH), dtype=torch.int32, device="cuda:0")
            times = []
            for round_ in range(warmup + repeats):
                begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                begin.record()
                tracer.tonemap_device(WIDTH, HEIGHT, frame.data_ptr(), state.data_ptr(), params, rgb.data_ptr(), rgba.data_ptr(), stream=stream)
                end.record()
                end.synchronize()
                if round_ >= warmup:
                    times.append(begin.elapsed_time(end))
            words = state.cpu().numpy().view(np.uint32)
            out.update(exposure=float(words[:1].view(np.float32)[0]), counted=int(words[2]), skipped=int(words[3]), kept=int(words[4]), mean_q8=int(words[5]), bytes_moved=WIDTH * HEIGHT * (12 + 12 + 12 + 4),
                       note="events around the fills and the launches of one call; bytes: the frame read twice, the float and the packed frame written")
        else:
            pod = lights_scene(tracer)
            times = []
            for round_ in range(warmup + repeats):
                if kind == "render":
                    _, _, stats = tracer.render(pod, WIDTH, HEIGHT, seed=SEED + round_, flags=capi.RT_HIP_FLAG_EMISSION)
                else:
                    _, _, stats, info = tracer.render_tonemapped(pod, WIDTH, HEIGHT, seed=SEED + round_, flags=capi.RT_HIP_FLAG_EMISSION)
                if round_ >= warmup:
                    times.append(stats["render_ms"])
            out.update(spp=SPP, lights=LIGHTS, primary_samples=stats["primary_samples"], kernel=stats["kernel"])
            if kind == "tonemapped":
                out.update(**info)
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
