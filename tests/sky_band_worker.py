"""Child process of tests/test_gpu_sky_band.py: renders the cases of a spec on GPU 0 with whatever RT_HIP_SKY_BAND says in ITS
environment (the knob is read when the context is created), and leaves frames, float means and counters in an .npz.

    python tests/sky_band_worker.py <spec.json> <out.npz>

Each case of the spec: {"name", "toml" or "scene" (a named scene), "camera" (position, direction) or null, "spp", "width", "height",
"seed", "flags"}; `"device": true` renders through rt_hip_render_device into device buffers instead of the drop-in call; `"then_pass": true`
renders the same frame once more right behind it as ONE pass over all samples with the camera unmoved — rt_hip_render_progressive behind
the drop-in call, rt_hip_render_pass_device onto a zeroed accumulator behind the device-level one — and keeps that frame too."""
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

import rt_amd  # noqa: E402


def scene_of(case):
    scene = rt_amd.Scene.parse(case["toml"]) if case.get("toml") else rt_amd.Scene.named(case["scene"])
    if case.get("camera"):
        scene.set_camera(*case["camera"])
    return scene.set_sampling(samples_per_pixel=case["spp"])


def main(spec_path, out_path):
    cases = json.loads(Path(spec_path).read_text())
    results = {}
    with rt_amd.HipRayTracer(device=0) as tracer:
        for case in cases:
            width, height = case["width"], case["height"]
            scene = scene_of(case)
            pod = scene.describe(width, height)
            print(f"case {case['name']}", file=sys.stderr, flush=True)  # (the band's own log lines follow it)
            if case.get("device"):
                import torch

                d_rgba = torch.zeros((height, width), dtype=torch.int32, device="cuda:0")
                d_rgb = torch.zeros((height, width, 3), dtype=torch.float32, device="cuda:0")
                tracer.upload(pod)
                tracer.render_device(width, height, d_rgba.data_ptr(), seed=case["seed"], flags=case["flags"], d_rgb_f32=d_rgb.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
                stats = tracer.stats()
                rgba, rgb = d_rgba.cpu().numpy().view(np.uint32), d_rgb.cpu().numpy()
                if case.get("then_pass"):
                    d_accum = torch.zeros((height, width, 3), dtype=torch.float32, device="cuda:0")
                    d_rgba.zero_(), d_rgb.zero_()
                    tracer.render_pass_device(width, height, 0, case["spp"], d_accum.data_ptr(), d_rgba.data_ptr(), seed=case["seed"], flags=case["flags"], d_rgb_f32=d_rgb.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
                    pass_stats = tracer.stats()
                    pass_rgba, pass_rgb = d_rgba.cpu().numpy().view(np.uint32), d_rgb.cpu().numpy()
            else:
                rgba, rgb, stats = tracer.render(pod, width, height, seed=case["seed"], flags=case["flags"], want_rgb=True)
                if case.get("then_pass"):
                    pass_rgba, pass_rgb, pass_stats, progress = tracer.render_progressive(pod, width, height, seed=case["seed"], flags=case["flags"], pass_samples=0, want_rgb=True)
                    assert progress["samples_done"] == case["spp"], progress
            if case.get("then_pass"):
                results[case["name"] + "/pass_rgba"] = pass_rgba
                results[case["name"] + "/pass_rgb"] = pass_rgb
                results[case["name"] + "/pass_counts"] = np.array([pass_stats["segments"], pass_stats["primary_samples"]], dtype=np.uint64)
            results[case["name"] + "/rgba"] = rgba
            results[case["name"] + "/rgb"] = rgb
            results[case["name"] + "/counts"] = np.array([stats["segments"], stats["primary_samples"]], dtype=np.uint64)
            results[case["name"] + "/kernel"] = np.array(str(stats["kernel"]))
    np.savez(out_path, **results)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
