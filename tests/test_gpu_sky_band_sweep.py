"""The sky band on the GPU along the axes tests/test_gpu_sky_band.py leaves narrow: the chunk count K = ceil(samples / 16),
the tile shape of the scene's kernel below the band, ragged widths, and the rule's kept answer.

Chunk count: the band kernel's four waves take four chunks a round, so only from K = 5 does its outer loop run a second round — the step
of four, the `parked` tail, the start value of a chunk that is not the frame's first, the barrier that protects the slots.  K here is
4, 5, 8, 16, 17, 32 and 256 (the one-shot limit: 64 rounds above, 48 KiB of chunk-sum slots below).

Tile shape: the scene's kernel is planned anew for H - R rows and told its first row; how its tiles are cut depends on K, on whole or
half chunks and on where the frame lives (page-locked memory behind rt_hip_render, HBM behind rt_hip_render_device).  Before a frame is
compared the CPU plan dump (tests/lds_plan.py) is asked for the plan below the band and the frame's build is held to what the case is
for; the last test prints, per build, the (K, pixels_log2, tile, HALF) the module's frames take and asserts that together they take all
ten tile shapes, and four-pixel tiles in half and in whole chunks on both tile-per-wave kernels.

Widths: 67 (ragged against tile widths 2, 4, 8 and 16; the band's last workgroup has three live lanes), 65 (one), 13 (less than one
band workgroup), 1.  The heights leave an odd number of rows below the band — ragged against tile heights 2, 4 and 8 — or three, or none.

Kept answers: render.hip keeps the rule's last answer per context.  A block of neighbouring frames that differ in ONE thing — the scene,
a flag, the sample count — and then go back is rendered on the same context: a stale answer would paint sky over a sphere.

As in tests/test_gpu_sky_band.py two child processes (tests/sky_band_worker.py) render every case once, one with RT_HIP_SKY_BAND=0 and
one without the variable.  Tolerance 0 against oracle.render, never against another GPU frame; the band's log line must show the rows
tests/test_sky_band_rule.py holds the rule to (SWEEP_ROWS, GPU_ROWS), and 0 in the run without."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from oracle import binding as oracle
from rt_amd import capi
from tests import lds_plan
from tests.conftest import ROOT
from tests.test_gpu_chunk_sweep import DEVICE_LDS, build_name, camera_of
from tests.test_sky_band_rule import GPU_ROWS, GPU_SCENES, SWEEP_ROWS, gpu_scene

pytestmark = pytest.mark.gpu

WHOLE = capi.RT_HIP_FLAG_FORCE_WHOLE_CHUNKS
RESIDENT = capi.RT_HIP_FLAG_FORCE_RESIDENT
BVH = capi.RT_HIP_FLAG_BVH
RAGGED = (67, 27)
# spp: K — one full round of the band kernel; a second round of one chunk of ONE sample (and the first four-pixel tiles below); two full
# rounds; the headline's build, the last HALF; the first whole-chunk build, a one-sample last chunk; a short last chunk; the limit
SAMPLES = {64: 4, 65: 5, 128: 8, 256: 16, 257: 17, 500: 32, 4096: 256}
# ... and under RT_HIP_FLAG_FORCE_WHOLE_CHUNKS three smaller counts as well: tiles of 32, 16 and 8 pixels in whole chunks
WHOLE_SAMPLES = {17: 2, 33: 3, 65: 5, 128: 8, 256: 16, 4096: 256}
EVERY_SIZE_AT = (65, 256, 257)  # K = 5, 16, 17
# pixels_log2 of a tile-per-wave tile by K (launch_plan.cpp), as the plan dump gives it for these counts: half chunks up to K = 16 unless whole are forced
PIXELS_LOG2 = {False: {1: 6, 2: 4, 3: 3, 4: 3, 5: 2, 8: 2, 16: 2, 17: 2, 32: 2, 256: 2}, True: {2: 5, 3: 4, 4: 4, 5: 3, 8: 3, 16: 2, 17: 2, 32: 2, 256: 2}}
HOST_TILES = {(16, 4), (16, 2), (16, 1), (8, 1), (4, 1)}  # rt_hip_render: rows of a page-locked frame
DEVICE_TILES = {(8, 8), (8, 4), (4, 4), (4, 2), (2, 2)}  # rt_hip_render_device: squares in HBM


def case_name(scene, flags, size, spp, seed, device=False):
    return f"{scene}-{flags:x}-{size[0]}x{size[1]}-{spp}spp-seed{seed}" + ("-device" if device else "")


def sweep_cases():
    cases = []
    for device in (False, True):
        for spp in SAMPLES:  # every (K, entry point) on the ragged frame, on both tile-per-wave kernels
            cases += [("basic", 0, RAGGED, spp, 1, device), ("basic", 0, RAGGED, spp, 2, device), ("many", 0, RAGGED, spp, 1, device)]
        for spp in WHOLE_SAMPLES:
            cases.append(("basic", WHOLE, RAGGED, spp, 1, device))
        for spp in (17, 33, 65, 256):
            cases.append(("many", WHOLE, RAGGED, spp, 1, device))
        for spp in (65, 256, 257, 4096):
            cases.append(("basic", RESIDENT, RAGGED, spp, 1, device))
        for scene, size in SWEEP_ROWS:  # every other size at K = 5, 16 and 17
            if (scene, size) not in (("basic", RAGGED), ("many", RAGGED)):
                for spp in EVERY_SIZE_AT:
                    cases.append((scene, 0, size, spp, 1, device))
    # a few more where the shapes meet the limits
    cases += [("basic", 0, (13, 43), 4096, 1, False), ("basic", WHOLE, (1, 40), 65, 1, False), ("basic", WHOLE, (1, 40), 33, 1, True), ("up", WHOLE, RAGGED, 33, 1, False), ("up", WHOLE, RAGGED, 17, 1, True),
              ("up", 0, (63, 24), 4096, 1, True), ("basic", RESIDENT, (65, 35), 128, 1, True), ("many", WHOLE, (13, 43), 65, 1, False)]
    return cases


CASES = sweep_cases()

# The kept answer: neighbours that differ in ONE field, on one context, at 200 x 113, seed 1, the scenes' own camera.
KEPT_SIZE = (200, 113)
KEPT = {  # name: ([(scene, flags, spp)], the one field that moves, the band's rows in the log)
    "scene": ([("basic", 0, 33), ("floating", 0, 33), ("basic", 0, 33)], 0, [48, 32, 48]),
    "flags": ([("many", 0, 33), ("many", BVH, 33), ("many", 0, 33)], 1, [48, 0, 48]),  # (RT_HIP_FLAG_BVH takes no band; a parity frame all the same)
    "samples": ([("basic", 0, 16), ("basic", 0, 33), ("basic", 0, 16)], 2, [48, 48, 48]),
}
KEPT_RUNS = [(name, device) for name in KEPT for device in (False, True)]


def kept_name(name, device, k):
    return f"kept-{name}-{k}" + ("-device" if device else "")


def kept_frames(name, device):
    """[(the case's name in the spec, (scene, flags, size, spp, seed, device))] of one sequence"""
    return [(kept_name(name, device, k), (scene, flags, KEPT_SIZE, spp, 1, device)) for k, (scene, flags, spp) in enumerate(KEPT[name][0])]


def spec_entry(name, scene, flags, size, spp, seed, device):
    named, toml, camera = GPU_SCENES[scene]
    return {"name": name, "scene": named, "toml": toml, "camera": camera, "spp": spp, "width": size[0], "height": size[1], "seed": seed, "flags": flags, "device": device, "then_pass": False}


def whole_spec():
    """every case of the sweep, then the kept-answer sequences: the worker renders them in this order on one context"""
    spec = [spec_entry(case_name(*case), *case) for case in CASES]
    for name, device in KEPT_RUNS:
        spec += [spec_entry(frame, *case) for frame, case in kept_frames(name, device)]
    assert len({entry["name"] for entry in spec}) == len(spec)
    return spec


def band_of(scene, flags, size):
    """the rows the rule gives the frame: tests/test_sky_band_rule.py holds both tables to it"""
    if flags & BVH:
        return 0
    return SWEEP_ROWS[(scene, size)] if (scene, size) in SWEEP_ROWS else GPU_ROWS[(scene, size[1])]


def plan_below_the_band(scene, flags, size, spp, device):
    """plan_launch as render.hip asks it for the rows below the band; None where there is none (R == H: no scene kernel is launched)"""
    rows = size[1] - band_of(scene, flags, size)
    if rows == 0:
        return None
    pod = gpu_scene(scene).describe(*size)
    return lds_plan.plan(pod.n_spheres, pod.n_planes, size[0], rows, spp, camera=camera_of(pod, *size), flags=flags, host_frame=0 if device else 1, lds_limit=DEVICE_LDS)


def tile_of(p):
    return (1 << p["tile_w_log2"], 1 << (p["pixels_log2"] - p["tile_w_log2"]))


def assert_the_plan_is_what_the_case_is_for(scene, flags, size, spp, device):
    p = plan_below_the_band(scene, flags, size, spp, device)
    if p is None:
        assert band_of(scene, flags, size) == size[1]
        return None
    pod = gpu_scene(scene).describe(*size)
    chunks, whole = -(-spp // 16), bool(flags & WHOLE)
    resident = bool(flags & RESIDENT) or pod.n_spheres > 8
    assert p["refusal"] == "" and p["slot_bytes"] <= p["max_slot_bytes"], p
    assert p["chunks"] == chunks and p["pixels_log2"] == PIXELS_LOG2[whole][chunks], (scene, flags, size, spp, p)
    assert p["halves"] == int(2 <= chunks <= 16 and not whole) and p["sub_chunk_items"] == p["halves"], p
    assert p["scan"] == (0 if resident else pod.n_spheres) and p["planes"] == 0 and not p["pass"] and not p["big_scene"], p
    assert tile_of(p) in (DEVICE_TILES if device else HOST_TILES), p
    assert p["tiles_x"] == -(-size[0] // tile_of(p)[0]) and p["tiles_y"] == -(-(size[1] - band_of(scene, flags, size)) // tile_of(p)[1]), p
    return p


def run_workers(folder, spec):
    """{"off": results, "on": results, "off_log" / "on_log": {case: [band rows of every launch]}}"""
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
def rendered(tmp_path_factory):
    return run_workers(tmp_path_factory.mktemp("sky_band_sweep"), whole_spec())


@pytest.fixture(scope="module")
def references():
    """the oracle's frame of a (scene, size, spp, seed), rendered once and left unchanged"""
    frames = {}

    def reference(scene, size, spp, seed):
        key = (scene, size, spp, seed)
        if key not in frames:
            pod = gpu_scene(scene).set_sampling(samples_per_pixel=spp).describe(*size)
            rgba, rgb, stats = oracle.render(pod, size[0], size[1], seed=seed)
            rgba.setflags(write=False), rgb.setflags(write=False)
            frames[key] = (rgba, rgb, stats["segments"])
        return frames[key]

    return reference


def assert_the_frame_is_the_oracles(rendered, references, name, case, rows):
    scene, flags, size, spp, seed, device = case
    want_rgba, want_rgb, want_segments = references(scene, size, spp, seed)
    # the run with the band took the rows the rule gives this frame; the run without took none
    assert rendered["on_log"].get(name) == [rows], (name, rendered["on_log"].get(name), rows)
    assert rendered["off_log"].get(name) == [0], (name, rendered["off_log"].get(name))
    for mode in ("off", "on"):
        got = rendered[mode]
        assert got[name + "/rgba"].shape == want_rgba.shape
        assert np.array_equal(got[name + "/rgba"], want_rgba), f"{name}, band {mode}: {(got[name + '/rgba'] != want_rgba).sum()} packed pixels differ from the oracle's (rows {sorted(set(np.nonzero(got[name + '/rgba'] != want_rgba)[0].tolist()))})"
        assert np.array_equal(got[name + "/rgb"].view(np.uint32), want_rgb.view(np.uint32)), f"{name}, band {mode}: float means differ from the oracle's (rows {sorted(set(np.nonzero(got[name + '/rgb'] != want_rgb)[0].tolist()))})"
    on, off = rendered["on"], rendered["off"]
    print(f"{name}: band {rows} of {size[1]} rows, segments {int(on[name + '/counts'][0])} (oracle {want_segments}), primary samples {int(on[name + '/counts'][1])}, kernel {on[name + '/kernel']}")
    assert np.array_equal(on[name + "/counts"], off[name + "/counts"]), (on[name + "/counts"], off[name + "/counts"])
    assert str(on[name + "/kernel"]) == str(off[name + "/kernel"])
    assert int(on[name + "/counts"][1]) == size[0] * size[1] * spp
    assert int(on[name + "/counts"][0]) == want_segments


@pytest.mark.parametrize("scene,flags,size,spp,seed,device", CASES, ids=[case_name(*c) for c in CASES])
def test_band_on_equals_band_off_equals_the_oracle(rendered, references, scene, flags, size, spp, seed, device):
    case = (scene, flags, size, spp, seed, device)
    assert_the_plan_is_what_the_case_is_for(scene, flags, size, spp, device)
    assert_the_frame_is_the_oracles(rendered, references, case_name(*case), case, SWEEP_ROWS[(scene, size)])


@pytest.mark.parametrize("name,device", KEPT_RUNS, ids=[f"{name}{'-device' if device else ''}" for name, device in KEPT_RUNS])
def test_a_kept_answer_is_not_used_for_another_frame(rendered, references, name, device):
    """A, then B, then A again on one context, B differing from A in one field: every frame takes ITS band and is the oracle's."""
    sequence, moves, rows = KEPT[name]
    frames = kept_frames(name, device)
    # the neighbours share everything but the one field — size, seed and entry point are the sequence's, the camera each scene's own
    assert GPU_SCENES["basic"][2] is None and GPU_SCENES["floating"][2] is None and GPU_SCENES["many"][2] is None
    for (_, before), (_, after) in zip(frames, frames[1:]):
        assert [k for k in range(6) if before[k] != after[k]] == [(0, 1, 3)[moves]], (before, after)
    assert frames[0][1] == frames[2][1]
    # (the worker renders the spec in order: the three frames are neighbours on the context)
    order = [entry["name"] for entry in whole_spec()]
    first = order.index(frames[0][0])
    assert order[first : first + 3] == [frame for frame, _ in frames]
    assert rows == [band_of(scene, flags, KEPT_SIZE) for scene, flags, _ in sequence]
    assert rows == {"scene": [48, 32, 48], "flags": [48, 0, 48], "samples": [48, 48, 48]}[name]
    for (frame, case), band in zip(frames, rows):
        scene, flags, size, spp, _, _ = case
        if band:
            assert_the_plan_is_what_the_case_is_for(scene, flags, size, spp, device)
        assert_the_frame_is_the_oracles(rendered, references, frame, case, band)


def test_the_cases_cover_what_they_are_for(capsys):
    """The plan dump asked once more for every frame of the module: per build the (K, pixels_log2, tile, HALF) taken below a band."""
    ran, tiles = {}, {False: set(), True: set()}
    kept = [case for name, device in KEPT_RUNS for _, case in kept_frames(name, device) if band_of(case[0], case[1], case[2])]
    for scene, flags, size, spp, _, device in CASES + kept:
        rows = band_of(scene, flags, size)
        assert rows > 0  # (no frame here is for a launch without a band)
        p = assert_the_plan_is_what_the_case_is_for(scene, flags, size, spp, device)
        if p is None:
            continue
        ran.setdefault((build_name(p), "HBM" if device else "page-locked"), set()).add((p["chunks"], p["pixels_log2"], tile_of(p), p["halves"], p["scan"]))
        tiles[device].add(tile_of(p))
    with capsys.disabled():
        print("\nbuild, destination: (K, pixels_log2, tile, HALF) of the frames of tests/test_gpu_sky_band_sweep.py below their bands")
        for build, where in sorted(ran):
            print(f"  {build}, {where}: " + ", ".join(f"({k}, {log2}, {w}x{h}, {half})" for k, log2, (w, h), half, _ in sorted(ran[(build, where)])))
    # all ten tile shapes, each where its entry point cuts it
    assert tiles[False] == HOST_TILES and tiles[True] == DEVICE_TILES, tiles
    # four-pixel tiles in half chunks and in whole chunks, on the scalar-register and on the LDS-resident kernel, from both entry points
    cells = {(where, scan > 0, half) for (_, where), taken in ran.items() for _, log2, _, half, scan in taken if log2 == 2}
    assert cells == {(where, registers, half) for where in ("HBM", "page-locked") for registers in (False, True) for half in (0, 1)}, cells
    # every (K, entry point) on the ragged frame of both kernels' scenes; every other size at K = 5, 16, 17 from both entry points
    for scene in ("basic", "many"):
        for device in (False, True):
            assert {-(-spp // 16) for s, flags, size, spp, _, d in CASES if (s, flags, size, d) == (scene, 0, RAGGED, device)} == set(SAMPLES.values()) == {4, 5, 8, 16, 17, 32, 256}
    for scene, size in SWEEP_ROWS:
        for device in (False, True):
            assert {5, 16, 17} <= {-(-spp // 16) for s, flags, sz, spp, _, d in CASES if (s, flags, sz, d) == (scene, 0, size, device)}, (scene, size, device)
    assert {seed for s, _, size, _, seed, _ in CASES if (s, size) == ("basic", RAGGED)} == {1, 2}
    # the widths and heights: three lanes, one lane, less than a workgroup, one column; an odd number of rows below, three, none
    assert {size for _, _, size, *_ in CASES} == {(67, 27), (13, 43), (1, 40), (65, 35), (63, 24)}
    assert {(size[0] % 64, size[1] - SWEEP_ROWS[(scene, size)]) for scene, _, size, *_ in CASES} == {(3, 19), (13, 27), (1, 24), (1, 19), (3, 3), (63, 0)}
    # the limit: 64 rounds of the band kernel above 48 KiB of chunk-sum slots
    p = plan_below_the_band("basic", 0, RAGGED, 4096, False)
    assert (p["chunks"], p["slot_bytes"]) == (256, 48 * 1024)
