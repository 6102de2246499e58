"""The launch policy (rt_amd/csrc/launch_plan.cpp: which kernel, which build of it, tile shape, sub-chunk items, sparse launches,
grid, LDS, HBM buffers) on the CPU.  A wrong threshold costs speed, not bits, so no parity test sees it: this one pins every decision.

tests/native/launch_plan_dump.cpp and launch_plan.cpp are built with g++ alone — nothing of ROCm on the command line, which is the
proof that the policy is host-only — and every request of the grid below must come out as tests/golden/launch_plans.txt says.  The
table was recorded when the functions had only been moved out of kernels.hip, bodies unchanged, and plan_launch was the plain
composition of what render.hip and launch_render used to work out separately.  Next to it, the invariants the kernels rely on.

queue_params::block_items, lane_cap, sparse_rays and item_samples are fields of the rolling (big-scene) kernels: choose_queue sets
them for those launches only and the other kernels never read them.  Their invariants are asserted for every rolling row; in every
other row they must be 0, as choose_queue leaves them."""
import shutil
import subprocess

import pytest

from rt_amd import capi
from tests.conftest import ROOT

SOURCES = [str(ROOT / "tests" / "native" / "launch_plan_dump.cpp"), str(ROOT / "rt_amd" / "csrc" / "launch_plan.cpp")]
KERNEL = {name: code for code, name in capi.KERNEL_NAMES.items()}  # RT_HIP_KERNEL_*
GOLDEN = ROOT / "tests" / "golden" / "launch_plans.txt"

SAMPLES = [1, 2, 8, 9, 16, 17, 32, 64, 112, 113, 256, 1000, 4096]
FRAMES = [(1, 1), (64, 36), (240, 135), (800, 600), (1280, 720), (1920, 135), (1920, 1080), (3840, 2160)]
SCENES = [(1, 0), (4, 0), (4, 1), (5, 3), (7, 1), (8, 0), (0, 1), (9, 0), (12, 1), (39, 0), (40, 0), (700, 2), (1024, 0), (1025, 0), (1300, 0), (1301, 0), (2000, 0), (8192, 0), (100000, 0)]
# (spheres, planes, planes_tame): both ways where there are planes
SCENES_TAME = [(s, p, 1) for s, p in SCENES] + [(s, p, 0) for s, p in SCENES if p]
CAMERAS = [0, 1, 2]  # camera_form: pinhole, plain eye form, other
HOST = [0, 1]
FLAGS = [0, capi.RT_HIP_FLAG_SM_MATERIALS, capi.RT_HIP_FLAG_FAST, capi.RT_HIP_FLAG_BVH, capi.RT_HIP_FLAG_FORCE_TILED, capi.RT_HIP_FLAG_FORCE_RESIDENT,
         capi.RT_HIP_FLAG_FORCE_STREAMED, capi.RT_HIP_FLAG_FORCE_HALF_CHUNKS, capi.RT_HIP_FLAG_FORCE_WHOLE_CHUNKS]
AXES = {"samples": SAMPLES, "frame": FRAMES, "scene": SCENES_TAME, "camera": CAMERAS, "host": HOST, "flags": FLAGS}
DEFAULT = {"samples": 64, "frame": (1920, 1080), "scene": (4, 0, 1), "camera": 0, "host": 0, "flags": 0}


def request(samples, frame, scene, camera, host, flags):
    fast = 1 if flags & capi.RT_HIP_FLAG_FAST else 0  # (as render.hip fills the request)
    return (scene[0], scene[1], scene[2], frame[0], frame[1], samples, camera, flags, host, fast)


def grid():
    """The cross product, thinned: the axes that meet in one decision are crossed in full, the others rotate through their values
    (a different one in every row, so that every pair of values turns up somewhere).  Deterministic; order is the fixture's."""
    turn = [0]

    def others(**fixed):
        turn[0] += 1
        row = {}
        for i, (axis, values) in enumerate(AXES.items()):
            if axis in fixed:
                row[axis] = fixed[axis]
            else:
                choice = [v for v in values if v != DEFAULT[axis]]  # never the default: see test_every_value_meets_non_default_company
                row[axis] = choice[(turn[0] * (2 * i + 3) + i) % len(choice)]
        return request(**row)

    rows = []
    # every value of every axis, in the company of non-default values on all other axes
    for axis, values in AXES.items():
        rows += [others(**{axis: v}) for v in values]
    # samples x frame (chunks per lane of the device, tile shapes, half chunks) for a scalar-register scene, the destination alternating,
    # and over four frames for a resident one
    rows += [request(spp, frame, (4, 0, 1), 0, (i + j) % 2, 0) for i, spp in enumerate(SAMPLES) for j, frame in enumerate(FRAMES)]
    rows += [request(spp, frame, (700, 2, 1), 0, (i + j + 1) % 2, 0) for i, spp in enumerate(SAMPLES) for j, frame in enumerate([(64, 36), (800, 600), (1920, 135), (1920, 1080)])]
    # scene x flags (which kernel, which build), scene x camera
    rows += [others(scene=scene, flags=flags) for scene in SCENES_TAME for flags in FLAGS]
    rows += [others(scene=scene, camera=camera) for scene in SCENES_TAME for camera in CAMERAS]
    # the big scenes' sub-chunk items, sparse and dense launches, and the resident kernel's last scenes: scene x samples, a small and a full frame
    rows += [request(spp, frame, (n, 0, 1), 1, 0, 0) for n in [1025, 1300, 2000, 8192, 100000] for spp in SAMPLES for frame in [(240, 135), (1920, 1080)]]
    return list(dict.fromkeys(rows))


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("launch_plan") / "launch_plan_dump"
    built = subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", *SOURCES, "-o", str(exe)], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr

    def run(requests):
        out = subprocess.run([str(exe)], input="".join(" ".join(str(v) for v in r) + "\n" for r in requests), capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr
        return out.stdout

    return run


def parse(table):
    lines = table.splitlines()
    assert lines[0].startswith("# ")
    names = [n for n in lines[0][2:].split() if n != "|"]
    rows = [dict(zip(names, (int(v) for v in line.split() if v != "|"))) for line in lines[1:]]
    assert all(len(r) == len(names) for r in rows)
    return rows


def test_every_value_meets_non_default_company():
    """Every value of every axis appears in at least one row in which every other axis is off its default."""
    rows = grid()
    columns = {"samples": lambda r: r[5], "frame": lambda r: (r[3], r[4]), "scene": lambda r: (r[0], r[1], r[2]), "camera": lambda r: r[6], "host": lambda r: r[8], "flags": lambda r: r[7]}
    for axis, values in AXES.items():
        for v in values:
            assert any(columns[axis](r) == v and all(columns[o](r) != DEFAULT[o] for o in AXES if o != axis) for r in rows), (axis, v)
    assert len(rows) < 800  # (a readable fixture)


def test_plans_are_the_recorded_ones(dump):
    got = dump(grid())
    want = GOLDEN.read_text()
    if got != want:
        g, w = got.splitlines(), want.splitlines()
        first = next((i for i, (a, b) in enumerate(zip(g, w)) if a != b), min(len(g), len(w)))
        pytest.fail(f"{sum(a != b for a, b in zip(g, w)) + abs(len(g) - len(w))} of {len(w)} rows differ; first at line {first + 1}:\n got  {g[first] if first < len(g) else None}\n want {w[first] if first < len(w) else None}")


def row_invariants(r):
    """What the kernels rely on in one row of the dump (tests/test_plan_frame_extremes.py holds its frames to the same)."""
    where = str(r)
    rolling = r["variant"] in (KERNEL["tiled"], KERNEL["streamed"])
    assert rolling == bool(r["big_scene"]) == (r["scan"] in (-1, -2, -3)) == (r["persistent_slot"] >= 0), where
    # tiles cover the rows, and are no wider than they are large
    tile_w_log2, tile_h_log2 = r["tile_w_log2"], r["pixels_log2"] - r["tile_w_log2"]
    assert r["tile_w_log2"] <= r["pixels_log2"], where
    assert (r["tiles_x"] << tile_w_log2) >= r["width"] and (r["tiles_y"] << tile_h_log2) >= r["local_rows"], where
    if rolling:
        assert 1 <= r["lane_cap"] <= 64, where
        assert 1 <= r["block_items"] <= max(r["lane_cap"], 8), where
        assert r["item_samples"] & (r["item_samples"] - 1) == 0 and 1 <= r["item_samples"] <= r["sample_chunk"], where
    else:  # (fields of the rolling kernels: not set, not read)
        assert r["lane_cap"] == r["block_items"] == r["item_samples"] == r["sparse_rays"] == 0, where
    if r["sm_table"] or r["flags"] & capi.RT_HIP_FLAG_FORCE_WHOLE_CHUNKS:
        assert r["halves"] == 0, where
    assert r["sub_chunk_items"] == r["halves"], where
    one_whole_chunk = r["chunks"] <= 1 and not r["halves"]
    assert (r["item_sums_bytes"] == 0) == (not rolling or one_whole_chunk), where
    assert (r["pixel_done_bytes"] == 0) == (r["item_sums_bytes"] == 0), where
    assert r["lds_bytes"] == r["table_bytes"] + r["slot_bytes"], where
    if not rolling:
        assert r["slot_bytes"] == r["four_tile_slot_bytes"] and r["lds_bytes"] == r["table_bytes"] + r["four_tile_slot_bytes"], where
        assert (r["grid_x"], r["grid_y"]) == ((r["tiles_x"] + 3) // 4, r["tiles_y"]), where
    else:
        assert r["slot_bytes"] == 0 and r["grid_y"] == 1 and 1 <= r["grid_x"] <= r["total_items"], where
        assert 0 <= r["persistent_slot"] < 18 and r["per_cu_cap"] == (6 if r["scan"] == -3 else 5), where
    if r["scan"] > 0:  # the scalar-register kernels: the builds that exist
        assert r["variant"] == KERNEL["small"] and (r["scan"], r["planes"]) == (r["n_spheres"], r["n_planes"]) and r["scan"] + r["planes"] <= 8 and r["planes"] <= 3, where


def test_invariants_the_kernels_rely_on(dump):
    rows = parse(dump(grid()))
    assert len(rows) == len(grid())
    seen = set()
    for r in rows:
        row_invariants(r)
        seen.add((r["variant"], r["scan"], r["planes"] if r["scan"] <= 0 else 0, r["general_camera"], r["halves"]))
    # the grid reaches every kernel, every scan mode and both item sizes
    assert {v for v, *_ in seen} == {KERNEL["resident"], KERNEL["tiled"], KERNEL["small"], KERNEL["streamed"], KERNEL["bvh"]}
    assert {s for _, s, *_ in seen if s <= 0} == {0, -1, -2, -3, -4}
    assert {(p, g) for _, s, p, g, _ in seen if s == 0} == {(0, 0), (0, 1), (1, 0)}
    assert any(r["lane_cap"] < 64 for r in rows if r["big_scene"]) and any(r["halves"] for r in rows if r["big_scene"]) and any(r["halves"] for r in rows if not r["big_scene"])


def test_a_frame_without_rows_launches_nothing(dump):
    """A rank whose share of the frame is empty: RT_HIP_KERNEL_NONE, no items, no buffers, whatever the scene."""
    for r in parse(dump([request(64, (1920, 0), scene, 0, 0, 0) for scene in [(4, 0, 1), (700, 2, 1), (8192, 0, 1)]])):
        assert r["variant"] == KERNEL["none"] and r["total_items"] == 0 and r["item_sums_bytes"] == 0 and r["pixel_done_bytes"] == 0
