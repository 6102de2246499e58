"""The sky band on the GPU: a frame rendered with the band — its upper rows by the scene-free kernel of sky_band.hip,
the rest by the scene's kernel over fewer rows — is the frame rendered without it and the oracle's, bit for bit: packed pixels, float
means, segment and sample counts.

RT_HIP_SKY_BAND is read when a context is created, so the two renderings come from two child processes (tests/sky_band_worker.py),
one with RT_HIP_SKY_BAND=0 and one without the variable; both run once for the whole module and render every case.  The band's log
line (RT_HIP_SKY_BAND_LOG=1) must show the rows tests/test_sky_band_rule.py holds the rule to — a comparison of two frames that both
took no band would prove nothing."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from oracle import binding as oracle
from rt_amd import capi
from tests.conftest import ROOT
from tests.test_sky_band_rule import GPU_ROWS, GPU_SCENES, GPU_SIZES, gpu_scene

pytestmark = pytest.mark.gpu

SAMPLES = [1, 16, 17, 33]  # the sample-0 rule alone, one whole chunk, a short last chunk, an odd chunk count
SEEDS = [1, 2]
VARIANTS = [("basic", 0), ("basic", capi.RT_HIP_FLAG_FORCE_RESIDENT), ("dielectric", 0), ("up", 0), ("floating", 0)]
# a few more through other launches of the same kernels: half-chunk items, and the device-level entry point
EXTRA = [("basic", capi.RT_HIP_FLAG_FORCE_HALF_CHUNKS, 33, False), ("basic", 0, 33, True), ("up", 0, 17, True), ("many", 0, 33, False), ("many", 0, 33, True)]
# A one-shot frame and then, camera unmoved, ONE pass over all samples of the same frame: of a scene of more than 8 spheres both are planned
# onto the LDS-resident kernel with the same frame constants, so whatever the one-shot frame's band leaves behind on the context is there
# for the pass to trip over — a pass takes no band.  Through the drop-in calls and through the device-level ones.
THEN_PASS = {("many", 0, 33, False), ("many", 0, 33, True), ("basic", 0, 33, True)}


def case_name(scene, flags, size, spp, seed, device=False):
    return f"{scene}-{flags:x}-{size[0]}x{size[1]}-{spp}spp-seed{seed}" + ("-device" if device else "")


def all_cases():
    cases = []
    for scene, flags in VARIANTS:
        for size in GPU_SIZES:
            for spp in SAMPLES:
                for seed in SEEDS:
                    cases.append((scene, flags, size, spp, seed, False))
    for scene, flags, spp, device in EXTRA:
        for size in GPU_SIZES:
            cases.append((scene, flags, size, spp, 1, device))
    return cases


CASES = all_cases()


@pytest.fixture(scope="module")
def rendered(tmp_path_factory):
    """{"off": results, "on": results, "log": {case: band rows of the run with the band}}"""
    folder = tmp_path_factory.mktemp("sky_band")
    spec = []
    for scene, flags, size, spp, seed, device in CASES:
        named, toml, camera = GPU_SCENES[scene]
        spec.append({"name": case_name(scene, flags, size, spp, seed, device), "scene": named, "toml": toml, "camera": camera, "spp": spp, "width": size[0], "height": size[1], "seed": seed, "flags": flags, "device": device, "then_pass": (scene, flags, spp, device) in THEN_PASS})
    (folder / "spec.json").write_text(json.dumps(spec))
    out = {}
    for mode in ("off", "on"):
        env = {k: v for k, v in os.environ.items() if k != "RT_HIP_SKY_BAND"}
        env["RT_HIP_SKY_BAND_LOG"] = "1"
        if mode == "off":
            env["RT_HIP_SKY_BAND"] = "0"
        done = subprocess.run([sys.executable, str(ROOT / "tests" / "sky_band_worker.py"), str(folder / "spec.json"), str(folder / f"{mode}.npz")], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert done.returncode == 0, done.stdout + done.stderr
        out[mode] = dict(np.load(folder / f"{mode}.npz"))
        rows, case = {}, None
        for line in done.stderr.splitlines():
            if line.startswith("case "):
                case = line[5:]
            found = re.match(r"rt_hip sky band: rows (\d+) of (\d+)", line)
            if found:
                rows.setdefault(case, []).append(int(found.group(1)))
        out[mode + "_log"] = rows
    return out


@pytest.fixture(scope="module")
def references():
    """the oracle's frame of every (scene, size, spp, seed), rendered once"""
    frames = {}
    for scene, _, size, spp, seed, _ in CASES:
        key = (scene, size, spp, seed)
        if key not in frames:
            pod = gpu_scene(scene).set_sampling(samples_per_pixel=spp).describe(*size)
            frames[key] = oracle.render(pod, size[0], size[1], seed=seed)
    return frames


@pytest.mark.parametrize("scene,flags,size,spp,seed,device", CASES, ids=[case_name(*c) for c in CASES])
def test_band_on_equals_band_off_equals_the_oracle(rendered, references, scene, flags, size, spp, seed, device):
    name = case_name(scene, flags, size, spp, seed, device)
    want_rgba, want_rgb, want_stats = references[(scene, size, spp, seed)]
    # the run with the band took the rows the rule gives this scene; the run without took none
    then_pass = (scene, flags, spp, device) in THEN_PASS
    assert rendered["on_log"][name] == [GPU_ROWS[(scene, size[1])]] + [0] * then_pass, rendered["on_log"].get(name)
    assert rendered["off_log"][name] == [0] + [0] * then_pass
    for mode in ("off", "on"):
        got = rendered[mode]
        assert np.array_equal(got[name + "/rgba"], want_rgba), f"{name}, band {mode}: {(got[name + '/rgba'] != want_rgba).sum()} packed pixels differ from the oracle's"
        assert np.array_equal(got[name + "/rgb"].view(np.uint32), want_rgb.view(np.uint32)), f"{name}, band {mode}: float means differ from the oracle's"
    on, off = rendered["on"], rendered["off"]
    print(f"{name}: segments {int(on[name + '/counts'][0])} (oracle {want_stats['segments']}), primary samples {int(on[name + '/counts'][1])}, kernel {on[name + '/kernel']}")
    assert np.array_equal(on[name + "/counts"], off[name + "/counts"])
    assert str(on[name + "/kernel"]) == str(off[name + "/kernel"])
    assert int(on[name + "/counts"][1]) == size[0] * size[1] * spp
    if then_pass:  # the pass behind the frame: the same frame again, from a launch that took no band
        for mode in ("off", "on"):
            got = rendered[mode]
            assert np.array_equal(got[name + "/pass_rgba"], want_rgba), f"{name}, band {mode}: the pass behind the frame differs from the oracle in {(got[name + '/pass_rgba'] != want_rgba).sum()} packed pixels"
            assert np.array_equal(got[name + "/pass_rgb"].view(np.uint32), want_rgb.view(np.uint32)), f"{name}, band {mode}: the pass's float means differ from the oracle's"
            assert np.array_equal(got[name + "/pass_counts"], on[name + "/counts"]), (mode, got[name + "/pass_counts"], on[name + "/counts"])


def test_the_cases_cover_what_they_are_for():
    assert any(GPU_ROWS[(scene, size[1])] == size[1] for scene, _, size, *_ in CASES)  # a frame that launches no scene kernel at all
    assert all(GPU_ROWS[(scene, size[1])] > 0 for scene, _, size, *_ in CASES)
    assert {size for _, _, size, *_ in CASES} == {(200, 113), (64, 40)}
