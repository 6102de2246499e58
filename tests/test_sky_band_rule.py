"""The sky band's rule (rt_amd/csrc/sky_band.cpp) on the CPU: how many rows from the top of a frame PROVABLY see nothing.

tests/native/sky_band_dump.cpp, sky_band.cpp and frame_setup.cpp are built with g++ alone — nothing of ROCm on the command line, which is
the proof that the rule is host-only.  Soundness is held by brute force against the oracle: for every pixel of the rows a case claims,
primary rays through oracle.primary_ray — jitter numerators 0, 2^23 and 2^24 - 1 in both axes, and eight random pairs — must all be
misses of oracle.closest_hit.  The rule may claim fewer rows than are sky, never one that is not."""
import shutil
import struct
import subprocess

import numpy as np
import pytest

import rt_amd
from oracle import binding as oracle
from rt_amd import capi
from rt_amd.scene import scene_from_arrays
from tests.conftest import ROOT

SOURCES = [str(ROOT / "tests" / "native" / "sky_band_dump.cpp"), str(ROOT / "rt_amd" / "csrc" / "sky_band.cpp"), str(ROOT / "rt_amd" / "csrc" / "frame_setup.cpp")]
SMALL, MIDDLE = (64, 36), (200, 113)
MATERIALS = [[0, 0.5, 0.5, 0.5, 1.0, 0.0, 0.0]]
GROUND = [0.0, -1000.0, 0.0, 1000.0, 0]
LEVEL = [(0.0, 0.0, -1.0), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0), (-1.0, 0.0, 0.0)]
UP = (0.0, 1.0, 0.0)
EXCLUDED_FLAGS = ["FAST", "PREVIEW", "TRACE_BOXES", "BOX_BVH", "EMISSION", "BVH", "SM_MATERIALS"]
SCAN_RESIDENT, SCAN_STREAMED = 0, -2  # (launch_plan.hpp)


# The scenes tests/test_gpu_sky_band.py renders with the band on and off, and the rows the rule gives them at that test's two sizes: the
# GPU test holds the band's log line to this table, this file holds the table to the rule.
FLOATING_TOML = (ROOT / "scenes" / "basic.toml").read_text().replace(
    "    { material = 2, position = [1, 0.5, 0] },", "    { material = 2, position = [1, 0.5, 0] },\n    { material = 1, position = [0.5, 1.5, -2], radius = 0.25 },"
)
assert FLOATING_TOML.count("radius = 0.25") == 1
# eleven spheres, no plane, the headline's camera: a one-shot frame AND a pass of it are planned onto the LDS-resident kernel
MANY_TOML = (ROOT / "scenes" / "basic.toml").read_text().replace(
    "    { material = 2, position = [1, 0.5, 0] },",
    "    { material = 2, position = [1, 0.5, 0] },\n" + "".join(f"    {{ material = {1 + i % 2}, position = [{-2.1 + 0.6 * i:.1f}, 0.2, {1.0 - 0.2 * (i % 3):.1f}], radius = 0.2 }},\n" for i in range(8)),
)
assert MANY_TOML.count("radius = 0.2 }") == 8
GPU_SIZES = [(200, 113), (64, 40)]
GPU_SCENES = {  # name: (named scene, toml, camera)
    "basic": ("basic", None, None),
    "dielectric": ("dielectric", None, None),
    "up": ("basic", None, ((0.0, 1.0, 3.0), UP)),  # every row is sky: R == H where H is a whole number of strips
    "floating": (None, FLOATING_TOML, None),  # a sphere above the horizon cuts the band
    "many": (None, MANY_TOML, None),
}
GPU_ROWS = {("basic", 113): 48, ("dielectric", 113): 24, ("up", 113): 112, ("floating", 113): 32, ("basic", 40): 16, ("dielectric", 40): 8, ("up", 40): 40, ("floating", 40): 8,
            ("many", 113): 48, ("many", 40): 16}

# The frames of tests/test_gpu_sky_band_sweep.py, tiny and ragged on purpose, and the rows the rule gives them: (scene, (W, H)) -> R.
# 67 x 27: 67 is ragged against tile widths 2, 4, 8 and 16 and leaves the last band workgroup three lanes; 19 (or, looking up, 3) rows
# stay below the band.  13 x 43: narrower than one band workgroup.  1 x 40: one column.  65 x 35: the last band workgroup has one lane.
# 63 x 24, looking up: every row is sky at a height that is a whole number of strips — no scene kernel is launched.
SWEEP_ROWS = {("basic", (67, 27)): 8, ("many", (67, 27)): 8, ("basic", (13, 43)): 16, ("many", (13, 43)): 16, ("basic", (1, 40)): 16, ("basic", (65, 35)): 16,
              ("up", (67, 27)): 24, ("up", (63, 24)): 24}


def gpu_scene(name):
    named, toml, camera = GPU_SCENES[name]
    scene = rt_amd.Scene.parse(toml) if toml else rt_amd.Scene.named(named)
    return scene.set_camera(*camera) if camera else scene


def bits(x) -> int:
    return struct.unpack("<I", struct.pack("<f", float(x)))[0]


def matrix_of(position, direction, width, height):
    pod = rt_amd.Scene.named("basic").set_camera(position, direction).describe(width, height)
    return np.array(list(pod.inverse_view_projection), dtype=np.float32).reshape(4, 4)


def scene_of(spheres, position, direction, size):
    return scene_from_arrays(spheres=spheres, materials=MATERIALS, inverse_view_projection=matrix_of(position, direction, *size))


def request_line(pod, size, flags=0, is_pass=0, adaptive=0, scan=None, n_planes=0, rank=0, world=1, kind="band"):
    """one line of sky_band_dump's input: the sphere table as the kernels read it, (c, r^2) with the radius squared in binary32"""
    words = " ".join(f"{bits(v):x}" for v in pod.inverse_view_projection)
    table = []
    for i in range(pod.n_spheres):
        radius = np.float32(pod.sphere_radius[i])
        table += [pod.sphere_center_x[i], pod.sphere_center_y[i], pod.sphere_center_z[i], radius * radius]
    scan = (pod.n_spheres if 1 <= pod.n_spheres <= 8 else SCAN_RESIDENT) if scan is None else scan
    return f"{kind} {flags:x} {is_pass} {adaptive} {scan} {n_planes} {size[0]} {size[1]} {rank} {world} 8 64 8 {words} {pod.n_spheres} " + " ".join(f"{bits(v):x}" for v in table)


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("sky_band") / "sky_band_dump"
    # (no include path but the sources' own relative ones: no HIP header can be found)
    built = subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", *SOURCES, "-o", str(exe)], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr

    def run(lines):
        out = subprocess.run([str(exe)], input="".join(line + "\n" for line in lines), capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr
        got = out.stdout.splitlines()
        assert len(got) == len(lines)
        return [dict(field.split("=") for field in line.split()[1:]) for line in got]

    return run


def band_rows(dump, pod, size, **gates) -> int:
    rows = int(dump([request_line(pod, size, **gates)])[0]["rows"])
    assert rows % 8 == 0 and 0 <= rows <= size[1]
    return rows


def generated_cases():
    """seeded scenes of 1 to 8 spheres seen through axis-aligned cameras above a ground sphere, looking level or up"""
    rng = np.random.default_rng(20260121)
    cases = []
    for k in range(16):
        size = MIDDLE if k % 4 == 3 else SMALL
        position = (float(rng.uniform(-2, 2)), float(rng.uniform(0.6, 3.0)), float(rng.uniform(-2, 4)))
        direction = UP if k % 5 == 4 else LEVEL[k % 4]
        count = 1 + k % 8
        spheres = [GROUND] if k % 7 != 6 else []
        while len(spheres) < count:
            radius = float(rng.uniform(0.15, 0.8))
            floating = rng.uniform() < 0.3
            spheres.append([float(rng.uniform(-4, 4)), float(rng.uniform(1.5, 6.0)) if floating else radius, float(rng.uniform(-4, 4)), radius, 0])
        cases.append((f"generated-{k}", spheres, position, direction, size))
    return cases


def constructed_cases():
    eye, forward = (0.0, 1.0, 3.0), LEVEL[0]
    return [
        ("floating above the horizon", [GROUND, [0.5, 2.2, -2.0, 0.4, 0]], eye, forward, SMALL),
        ("behind the camera", [GROUND, [0.0, 1.5, 6.0, 1.0, 0]], eye, forward, SMALL),
        ("camera inside a sphere", [GROUND, [0.0, 1.0, 3.0, 2.0, 0]], eye, forward, SMALL),
        ("tangent to the horizontal plane through the eye", [GROUND, [0.3, 0.5, 0.0, 0.5, 0], [-1.0, 1.75, -1.0, 0.75, 0]], eye, forward, SMALL),
        ("far and tiny", [GROUND, [0.0, 1.0 + 1.0e4 * 0.1, 3.0 - 1.0e4 * 0.995, 0.5, 0]], eye, forward, SMALL),
        ("huge and near", [[0.0, -1.0e6, 0.0, 1.0e6, 0]], eye, forward, SMALL),
        ("huge and near, overhead", [GROUND, [0.0, 1.0e6 + 3.0, 0.0, 1.0e6, 0]], eye, forward, SMALL),
        ("straddling the near rectangle", [GROUND, [0.0, 1.0, 2.99, 0.004, 0]], eye, forward, SMALL),
    ]


def headline_cases():
    cases = []
    for size in (SMALL, MIDDLE):
        pod = rt_amd.Scene.named("basic").describe(*size)
        spheres = [[pod.sphere_center_x[i], pod.sphere_center_y[i], pod.sphere_center_z[i], pod.sphere_radius[i], 0] for i in range(pod.n_spheres)]
        cases.append((f"headline {size[0]}x{size[1]}", spheres, (0.0, 1.0, 3.0), LEVEL[0], size))
    return cases


def assert_rows_are_sky(pod, size, rows, name):
    """every pixel of rows [0, rows): the primary rays of eleven jitters all miss"""
    if not rows:
        return
    width = size[0]
    rng = np.random.default_rng(rows * 7919 + width)
    low, mid, high = 0.0, 2.0**23, 2.0**24 - 1.0
    fixed = [(low, low), (mid, mid), (high, high)]
    origins, directions = [], []
    for y in range(rows):
        for x in range(width):
            for ka, kb in fixed + [(float(a), float(b)) for a, b in rng.integers(0, 1 << 24, size=(8, 2))]:
                origin, direction = oracle.primary_ray(pod, size[0], size[1], x, y, ka, kb)
                origins.append(origin)
                directions.append(direction)
    _, kind, _, _ = oracle.closest_hit(pod, np.array(origins), np.array(directions))
    hits = np.flatnonzero(kind)
    assert hits.size == 0, f"{name}: the band claims {rows} rows, but {hits.size} of their rays hit something (the first: pixel {(int(hits[0]) // 11) % width, (int(hits[0]) // 11) // width})"


def test_claimed_rows_are_sky_for_every_jitter(dump):
    generated = generated_cases()
    claimed = {}
    for name, spheres, position, direction, size in generated + constructed_cases() + headline_cases():
        pod = scene_of(spheres, position, direction, size)
        assert int(dump([request_line(pod, size)])[0]["pinhole"]) == 1, name  # (an axis-aligned camera: the rule is asked in earnest)
        rows = band_rows(dump, pod, size)
        claimed[name] = rows
        assert_rows_are_sky(pod, size, rows, name)
    # not vacuous: at least half of the generated cases have a band
    assert sum(claimed[name] >= 8 for name, *_ in generated) * 2 >= len(generated), claimed
    # what must have no band at all, and what must have one
    assert claimed["camera inside a sphere"] == 0
    assert claimed["floating above the horizon"] < claimed["behind the camera"]
    assert claimed["behind the camera"] >= 8 and claimed["headline 200x113"] >= 40, claimed


def test_the_oracle_does_hit_below_the_band(dump):
    """the brute force above can fail: the row under the headline's band has pixels that hit"""
    size = MIDDLE
    pod = rt_amd.Scene.named("basic").describe(*size)
    origins, directions = zip(*(oracle.primary_ray(pod, size[0], size[1], x, size[1] - 1) for x in range(size[0])))
    _, kind, _, _ = oracle.closest_hit(pod, np.array(origins), np.array(directions))
    assert np.all(kind != 0)


def test_headline_band_at_full_size(dump):
    """scenes/basic.toml at 1920 x 1080: the horizontal is row 540, and the two small spheres top out exactly there"""
    pod = rt_amd.Scene.named("basic").describe(1920, 1080)
    rows = band_rows(dump, pod, (1920, 1080))
    assert 480 <= rows <= 540, rows
    assert rows == 536  # (DESIGN.md §5 states it)
    # ... and dielectric.toml's seven spheres, one of them above eye height
    pod = rt_amd.Scene.named("dielectric").describe(1920, 1080)
    assert 8 <= band_rows(dump, pod, (1920, 1080)) < 540


def test_gates(dump):
    size = MIDDLE
    pod = rt_amd.Scene.named("basic").describe(*size)
    assert band_rows(dump, pod, size) >= 40
    assert band_rows(dump, pod, size, scan=SCAN_RESIDENT) >= 40  # (the LDS-resident kernel is a tile-per-wave kernel too)
    assert band_rows(dump, pod, size, flags=capi.RT_HIP_FLAG_FORCE_HALF_CHUNKS | capi.RT_HIP_FLAG_STATS) >= 40
    for name in EXCLUDED_FLAGS:
        assert band_rows(dump, pod, size, flags=getattr(capi, f"RT_HIP_FLAG_{name}")) == 0, name
    assert band_rows(dump, pod, size, n_planes=1) == 0
    assert band_rows(dump, pod, size, world=2) == 0
    assert band_rows(dump, pod, size, world=2, rank=1) == 0
    assert band_rows(dump, pod, size, is_pass=1) == 0
    assert band_rows(dump, pod, size, is_pass=1, adaptive=1) == 0
    assert band_rows(dump, pod, size, scan=SCAN_STREAMED) == 0  # (a rolling kernel)
    tilted = rt_amd.Scene.named("basic").set_camera((1.0, 2.0, 3.0), (0.3, -0.2, -1.0)).describe(*size)
    answer = dump([request_line(tilted, size)])[0]
    assert int(answer["pinhole"]) == 0 and int(answer["rows"]) == 0


def test_non_finite_spheres_give_no_band(dump):
    size = SMALL
    for bad in (float("nan"), float("inf"), -float("inf")):
        for column in range(4):
            sphere = [0.0, 5.0, -20.0, 0.5, 0]
            sphere[column] = bad
            pod = scene_of([GROUND, sphere], (0.0, 1.0, 3.0), LEVEL[0], size)
            assert band_rows(dump, pod, size) == 0, (bad, column)


def test_rows_of_the_gpu_tests_scenes(dump):
    for name in GPU_SCENES:
        for size in GPU_SIZES:
            assert band_rows(dump, gpu_scene(name).describe(*size), size) == GPU_ROWS[(name, size[1])], (name, size)
            assert band_rows(dump, gpu_scene(name).describe(*size), size, scan=SCAN_RESIDENT) == GPU_ROWS[(name, size[1])], (name, size)
    assert GPU_ROWS[("up", 40)] == 40 and 0 < GPU_ROWS[("floating", 113)] < GPU_ROWS[("basic", 113)]


def test_rows_of_the_gpu_sweeps_frames(dump):
    """tests/test_gpu_sky_band_sweep.py holds the band's log line to SWEEP_ROWS; here the table is held to the rule, and the rule to the oracle."""
    for (name, size), rows in SWEEP_ROWS.items():
        pod = gpu_scene(name).describe(*size)
        assert band_rows(dump, pod, size) == rows, (name, size)
        assert band_rows(dump, pod, size, scan=SCAN_RESIDENT) == rows, (name, size)
        assert_rows_are_sky(pod, size, rows, f"{name} {size[0]}x{size[1]}")
    # what the GPU frames rely on: a band and an odd number of rows below it — ragged against every tile height — or no row below it at all
    for (name, size), rows in SWEEP_ROWS.items():
        if size in ((67, 27), (13, 43), (65, 35)):
            assert 0 < rows < size[1] and (size[1] - rows) % 2 == 1, (name, size, rows)
    assert SWEEP_ROWS[("up", (63, 24))] == 24 and SWEEP_ROWS[("up", (67, 27))] == 24 and 0 < SWEEP_ROWS[("basic", (1, 40))] < 40


def sanitizer_lines():
    """the input of `make sanitize-sky-band` (tests/golden/sky_band_cases.txt): cases of this file, gates and non-finite spheres included.
    `python -m tests.test_sky_band_rule` writes the file; test_the_sanitizer_input_is_this_files_cases holds it to this function."""
    lines = []
    for _, spheres, position, direction, size in generated_cases()[:6] + constructed_cases() + headline_cases():
        lines.append(request_line(scene_of(spheres, position, direction, size), size))
    for name in GPU_SCENES:
        for size in GPU_SIZES + [(1920, 1080)]:
            lines.append(request_line(gpu_scene(name).describe(*size), size))
    for name, size in SWEEP_ROWS:
        lines.append(request_line(gpu_scene(name).describe(*size), size))
        lines.append(request_line(gpu_scene(name).describe(*size), size, scan=SCAN_RESIDENT))
    pod = rt_amd.Scene.named("basic").describe(*MIDDLE)
    for flag in EXCLUDED_FLAGS:
        lines.append(request_line(pod, MIDDLE, flags=getattr(capi, f"RT_HIP_FLAG_{flag}")))
    lines += [request_line(pod, MIDDLE, n_planes=1), request_line(pod, MIDDLE, world=2, rank=1), request_line(pod, MIDDLE, is_pass=1), request_line(pod, MIDDLE, scan=SCAN_STREAMED)]
    lines.append(request_line(rt_amd.Scene.named("basic").set_camera((1.0, 2.0, 3.0), (0.3, -0.2, -1.0)).describe(*MIDDLE), MIDDLE))
    for bad in (float("nan"), float("inf")):
        lines.append(request_line(scene_of([GROUND, [0.0, bad, -20.0, 0.5, 0]], (0.0, 1.0, 3.0), LEVEL[0], SMALL), SMALL))
    lines.append(request_line(scene_of([], (0.0, 1.0, 3.0), LEVEL[0], SMALL), SMALL, scan=SCAN_RESIDENT))
    return list(dict.fromkeys(lines))  # (the headline is a case of several lists: once is enough)


def test_the_sanitizer_input_is_this_files_cases():
    assert (ROOT / "tests" / "golden" / "sky_band_cases.txt").read_text() == "".join(line + "\n" for line in sanitizer_lines())


if __name__ == "__main__":
    (ROOT / "tests" / "golden" / "sky_band_cases.txt").write_text("".join(line + "\n" for line in sanitizer_lines()))
