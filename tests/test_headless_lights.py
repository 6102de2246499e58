"""rt_headless --light (rt_amd/host/main.cpp): the option's argument checks without a GPU, and on one the frame the
plug-in renders from RT_HIP_LIGHTS — the scene's material names through rt_hip_lights_from_spec, rt_hip_set_emission and
RT_HIP_FLAG_EMISSION — against the CPU restatement."""
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT, unpack

BIN = ROOT / "rt_amd" / "bin" / "rt_headless"
LIGHTS = "tests/golden/scenes/lights.toml"
MESSAGE = "--light makes materials lights in one-shot frames of a hip renderer (not with --progressive, --adaptive, --temporal, --denoise or --boxes, not '"


def run(*args, **kw):
    return subprocess.run([str(BIN), *args], cwd=ROOT, capture_output=True, text=True, timeout=300, **kw)


@pytest.mark.parametrize("other", [("--progressive", "16"), ("--adaptive", "0.03"), ("--temporal",), ("--temporal", "--denoise"), ("--progressive", "16", "--denoise"), ("--boxes",), ("--boxes", "--box-bvh")])
def test_light_is_refused_with_the_options_that_have_no_light_build(other):
    out = run("--light", "lamp=4,3.2,2", *other, "--renderer", "hip", "--scene", LIGHTS, "--size", "16x8")
    assert out.returncode == 2 and ("error: " + MESSAGE + "hip_ray_tracer')") in out.stderr, out.stderr
    assert "created renderer" not in out.stdout  # nothing was created, nothing rendered


def test_light_is_refused_for_a_renderer_that_is_not_a_hip_one():
    out = run("--light", "lamp=1", "--renderer", "null", "--scene", LIGHTS, "--size", "16x8")
    assert out.returncode == 2 and ("error: " + MESSAGE + "null_renderer')") in out.stderr


def test_light_needs_a_value_and_is_in_the_usage_line():
    out = run("--light")
    assert out.returncode == 2 and "missing value for --light" in out.stderr
    assert "[--light KEY=R,G,B]..." in run("--help").stdout
    assert run("--list").stdout == run("--list", "--light", "lamp=1").stdout  # the registry's list, unchanged


@pytest.mark.gpu
@pytest.mark.parametrize("renderer,sm", [("hip_ray_tracer", False), ("hip_sm", True)])
def test_the_plugin_renders_the_restatements_frame(tmp_path, renderer, sm):
    """--light twice (the items joined with ';'): the lamp by name, the clay sphere by index."""
    from tests import light_reference as light_ref

    ppm = tmp_path / "frame.ppm"
    out = run("--renderer", renderer, "--scene", LIGHTS, "--size", "96x54", "--spp", "20", "--seed", "11", "--light", "lamp=4,3.2,2", "--light", "2=0.5", "--out", str(ppm))
    assert out.returncode == 0 and "error:" not in out.stderr, out.stderr
    header = b"P6\n96 54\n255\n"
    got = np.frombuffer(ppm.read_bytes()[len(header) :], dtype=np.uint8).reshape(54, 96, 3)
    table = light_ref.LIGHTS_TABLE.copy()
    table[2] = 0.5
    pod = light_ref.lights_scene(spp=20).describe(96, 54)
    want, _, _ = light_ref.render(pod, 96, 54, table, seed=11, want_rgb=False, sm_materials=sm)
    assert np.array_equal(got, unpack(want)[..., :3])


@pytest.mark.gpu
def test_a_malformed_spec_prints_an_error_and_leaves_the_cleared_frame(tmp_path):
    ppm = tmp_path / "frame.ppm"
    out = run("--renderer", "hip", "--scene", LIGHTS, "--size", "16x8", "--spp", "4", "--light", "lantern=1", "--out", str(ppm))
    assert "error: hip_ray_tracer: rt_hip_lights_from_spec: item 'lantern=1': no material of that name" in out.stderr
    header = b"P6\n16 8\n255\n"
    assert set(ppm.read_bytes()[len(header) :]) == {0}
