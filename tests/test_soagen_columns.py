"""SURVEY.md §8 row a-8 against the reference's own container runtime (VERDICT r2 "what's missing" #4).

`vendor/soagen.hpp` of the reference is std-only, so the build compiles it where it lies in the reference tree (Makefile:
oracle/_ref/soagen_columns, git-ignored): tests/native/soagen_columns.cpp builds `soagen::table`s with the column types, alignments and order of
the reference's `src/soa.toml` / `src/soa.hpp`, fills them, and hands the pointers the accessors return — 32-byte aligned
columns, capacity padded to 8-row strides, the padding rows poisoned — to the product's `rt_hip_scene_check` (pointer and
index check, column fingerprint: pure host code of librt_hip.so) and to the oracle's renderer.  Nothing of the reference
itself is read by the tests: where the build had no reference tree, the program does not exist and both tests skip.
"""
import subprocess

import pytest

from tests.conftest import ROOT

SOAGEN_EXE = ROOT / "oracle" / "_ref" / "soagen_columns"


def test_columns_of_a_real_soagen_table_are_read_up_to_size_and_no_further():
    if not SOAGEN_EXE.exists():
        pytest.skip("oracle/_ref/soagen_columns was not built (the build makes it only where the reference tree is present)")
    run = subprocess.run([str(SOAGEN_EXE)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.startswith("OK:"), run.stdout + run.stderr
    assert "11 spheres in capacity" in run.stdout  # padding rows existed (and were poisoned)


@pytest.mark.gpu
def test_real_soagen_columns_through_the_drop_in_call_on_the_gpu():
    """real `soagen::table` memory — 32-byte aligned columns, padded capacity, padding poisoned — handed to
    rt_hip_render on the GPU; the frame is the oracle's.  The program is built in the build container (Makefile:
    oracle/_ref/soagen_columns, from tests/native/soagen_columns.cpp and the reference's vendor/soagen.hpp in place) and travels
    to the GPU box as a binary."""
    exe = ROOT / "oracle" / "_ref" / "soagen_columns"
    if not exe.exists():
        pytest.skip("oracle/_ref/soagen_columns was not built (the build container has the reference tree; run `make` there)")
    run = subprocess.run([str(exe), "--gpu"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "OK:" in run.stdout, run.stdout + run.stderr
    assert run.stdout.count("equals the oracle's") == 2 and "DIFFERS" not in run.stdout, run.stdout
    assert "padding poisoned" in run.stdout


def test_scene_check_is_usable_without_a_gpu_and_agrees_with_the_loader():
    """rt_hip_scene_check on the scenes the host side loads: accepted, and the fingerprint only depends on the columns."""
    import numpy as np

    import rt_amd

    basic = rt_amd.Scene.named("basic")
    a = rt_amd.scene_check(basic.describe(64, 36))
    assert a == rt_amd.scene_check(basic.describe(1920, 1080))  # camera matrix and sampling are per-frame, not columns
    assert a == rt_amd.scene_check(basic.set_sampling(7, 3).describe(64, 36))
    assert a != rt_amd.scene_check(rt_amd.Scene.named("dielectric").describe(64, 36))
    pod = rt_amd.Scene.named("basic").describe(64, 36)
    radius = np.ctypeslib.as_array(pod.sphere_radius, shape=(pod.n_spheres,))
    radius[2] = np.nextafter(radius[2], np.float32(2))
    assert rt_amd.scene_check(pod) != a  # one ulp in one row
    with pytest.raises(rt_amd.RtHipError, match="out-of-range"):
        rt_amd.scene_check(rt_amd.scene_from_arrays(spheres=[(0, 0, -5, 1, 1)], materials=[(0, 1, 1, 1, 1, 0.5, 0.5)]))
    with pytest.raises(rt_amd.RtHipError, match="no materials"):
        rt_amd.scene_check(rt_amd.scene_from_arrays(spheres=[(0, 0, -5, 1, 0)]))
    # a column that moved in memory but holds the same rows keeps its fingerprint; an empty scene has one too
    rows = dict(spheres=[(0, 0, -5, 1, 0), (1, 0, -4, 0.5, 0)], planes=[(0, 1, 0, 0, 0)], materials=[(0, 1, 1, 1, 1, 0.5, 0.5)])
    assert rt_amd.scene_check(rt_amd.scene_from_arrays(**rows)) == rt_amd.scene_check(rt_amd.scene_from_arrays(**rows))
    assert rt_amd.scene_check(rt_amd.scene_from_arrays()) == rt_amd.scene_check(rt_amd.scene_from_arrays())
    moved = dict(rows, spheres=[(0, 0, -5, 1, 0)], planes=[(1, 0, -4, 0.5, 0), (0, 1, 0, 0, 0)])  # same floats, other columns
    assert rt_amd.scene_check(rt_amd.scene_from_arrays(**moved)) != rt_amd.scene_check(rt_amd.scene_from_arrays(**rows))
