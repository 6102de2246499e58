"""The sphere hierarchy of RT_HIP_FLAG_BVH, as built on the host (rt_hip_kat_bvh_build: no GPU).

What the traversal's "same answer as the linear scan" rests on, checked here on the builder's output: every sphere is in
exactly one leaf or in the always list, boxes contain what they must (node boxes the child boxes, leaf boxes the spheres'
boxes centre -/+ sqrt(r^2)), the depth stays within the traversal stack, the leaf table holds bit copies of the upload's
(c, r^2), and two builds are the same bytes.  The GPU side is tests/test_gpu_bvh.py."""
import re
import subprocess
import time

import numpy as np
import pytest

import rt_amd
from rt_amd import capi
from rt_amd.renderer import bvh_build
from tests.bvh_cases import STACK_DEPTH, check_tree, sphere_scene

ROOT = __import__("pathlib").Path(__file__).resolve().parent.parent


def header_constant(name):
    text = (ROOT / "rt_amd" / "csrc" / "bvh.hpp").read_text()
    return int(re.search(rf"constexpr uint32_t {name} = (\d+);", text).group(1))


def build_twice(scene):
    a, b = bvh_build(scene), bvh_build(scene)
    for key in ("nodes", "order", "spheres", "always", "bound"):
        assert a[key].tobytes() == b[key].tobytes(), f"two builds differ in {key}"
    assert (a["depth"], a["root"]) == (b["depth"], b["root"])
    return a


@pytest.mark.parametrize("count", [1500, 100000])
def test_synthetic_field(count):
    scene = rt_amd.Scene.synthetic(count).describe(64, 36)
    t0 = time.perf_counter()
    t = bvh_build(scene)
    seconds = time.perf_counter() - t0
    print(f"bvh build, {count} spheres: {seconds * 1e3:.1f} ms, {len(t['nodes'])} nodes, depth {t['depth']}, always list {list(t['always'])}")
    if count == 100000:
        assert seconds < 1.0
    check_tree(scene, t)
    # the ground sphere (radius 1000, sphere 0 of the field) stays out of the tree
    radius = np.ctypeslib.as_array(scene.sphere_radius, (count,))
    ground = int(np.argmax(radius))
    assert radius[ground] >= 100 and ground in set(t["always"].tolist())
    assert len(t["always"]) <= 8 + count // 256
    assert build_twice(scene)["nodes"].tobytes() == t["nodes"].tobytes()


@pytest.mark.parametrize("seed", range(200))
def test_random_scenes(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 600))
    spread = float(10 ** rng.uniform(-2, 3))
    rows = np.zeros((n, 5))
    rows[:, :3] = rng.normal(size=(n, 3)) * spread
    rows[:, 3] = np.abs(rng.normal(size=n)) * spread * float(10 ** rng.uniform(-3, 0))
    if seed % 5 == 0:
        rows[rng.integers(0, n)] = (0, -1000, 0, 1000, 0)
    check_tree(sphere_scene(rows), build_twice(sphere_scene(rows)))


DEGENERATE = {
    "one sphere": [(0, 0, -1, 0.5, 0)],
    "all identical": [(1, 2, 3, 0.5, 0)] * 64,
    "duplicates at one centre": [(0, 0, 0, 0.1 * (1 + i % 7), 0) for i in range(50)] + [(5, 0, 0, 0.2, 0)] * 30,
    "zero radius": [(float(i), 0, 0, 0.0, 0) for i in range(40)],
    "far apart": [(1e7 * (i % 3 - 1), 1e6 * (i % 5), -1e7 * (i % 2), 1.0, 0) for i in range(33)],
    "huge and tiny": [(0, -1e5, 0, 1e5, 0)] + [(i * 1e-3, 0, 0, 1e-5, 0) for i in range(100)] + [(0, 0, 0, 3e4, 0)],
    "negative radius": [(float(i), 0, 0, -0.25, 0) for i in range(20)],
    "not finite": [(np.nan, 0, 0, 1, 0), (0, np.inf, 0, 1, 0), (0, 0, 0, np.inf, 0), (1, 1, 1, 0.5, 0)] + [(float(i), 0, 2, 0.3, 0) for i in range(12)],
}


@pytest.mark.parametrize("name", list(DEGENERATE))
def test_degenerate_scenes(name):
    scene = sphere_scene(DEGENERATE[name])
    t = build_twice(scene)
    check_tree(scene, t)
    if name == "not finite":
        assert {0, 1, 2} <= set(t["always"].tolist())


def test_empty_scene():
    t = bvh_build(sphere_scene(np.zeros((0, 5))))
    assert len(t["order"]) == 0 and len(t["always"]) == 0 and len(t["nodes"]) == 0


def test_stack_capacity_matches_the_kernels():
    assert header_constant("bvh_max_depth") == STACK_DEPTH
    kernels = (ROOT / "rt_amd" / "csrc" / "launch_plan.hpp").read_text()  # (the kernels' LDS sizes live with the launch policy)
    assert re.search(r"bvh_stack_float4s = 24u \* 256u / 4u", kernels)


def test_flag_and_kernel_constants_match_the_header(tmp_path):
    """capi's RT_HIP_FLAG_BVH and RT_HIP_KERNEL_BVH against include/rt_hip.h as a C compiler sees it."""
    src = tmp_path / "probe.c"
    src.write_text('#include "rt_hip.h"\n#include <stdio.h>\nint main(void) { printf("%u %u %u\\n", (unsigned)RT_HIP_FLAG_BVH, (unsigned)RT_HIP_KERNEL_BVH, (unsigned)RT_HIP_ABI_VERSION); return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.run(["cc", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    flag, kernel, abi = (int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert (flag, kernel, abi) == (capi.RT_HIP_FLAG_BVH, capi.RT_HIP_KERNEL_BVH, capi.RT_HIP_ABI_VERSION)
    assert flag == 1 << 10 and kernel == 6 and abi == 6
    assert capi.KERNEL_NAMES[kernel] == "bvh"
