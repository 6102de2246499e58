"""rt_headless --direct-light (rt_amd/host/main.cpp): the option's argument checks without a GPU, and on one the frame
the plug-in renders from RT_HIP_LIGHTS and RT_HIP_DIRECT_LIGHT=1 — RT_HIP_FLAG_EMISSION | RT_HIP_FLAG_DIRECT_LIGHT — against the CPU
restatement."""
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT, unpack

BIN = ROOT / "rt_amd" / "bin" / "rt_headless"
LIGHTS = "tests/golden/scenes/lights.toml"
LIGHT_MESSAGE = "--light makes materials lights in one-shot frames of a hip renderer (not with --progressive, --adaptive, --temporal, --denoise or --boxes, not '"
DIRECT_MESSAGE = "--direct-light says how the lights of --light are found: lambert surfaces sample the sphere lights directly (not without --light)"


def run(*args, **kw):
    return subprocess.run([str(BIN), *args], cwd=ROOT, capture_output=True, text=True, timeout=300, **kw)


def test_direct_light_needs_light():
    out = run("--direct-light", "--renderer", "hip", "--scene", LIGHTS, "--size", "16x8")
    assert out.returncode == 2 and ("error: " + DIRECT_MESSAGE) in out.stderr, out.stderr
    assert "created renderer" not in out.stdout  # nothing was created, nothing rendered


@pytest.mark.parametrize("other", [("--progressive", "16"), ("--adaptive", "0.03"), ("--temporal",), ("--temporal", "--denoise"), ("--progressive", "16", "--denoise"), ("--boxes",), ("--boxes", "--box-bvh")])
def test_direct_light_is_refused_with_the_options_light_is_refused_with(other):
    """... in --light's own words, which stay as they are"""
    out = run("--light", "lamp=4,3.2,2", "--direct-light", *other, "--renderer", "hip", "--scene", LIGHTS, "--size", "16x8")
    assert out.returncode == 2 and ("error: " + LIGHT_MESSAGE + "hip_ray_tracer')") in out.stderr, out.stderr
    assert "created renderer" not in out.stdout


def test_direct_light_is_refused_for_a_renderer_that_is_not_a_hip_one():
    out = run("--light", "lamp=1", "--direct-light", "--renderer", "null", "--scene", LIGHTS, "--size", "16x8")
    assert out.returncode == 2 and ("error: " + LIGHT_MESSAGE + "null_renderer')") in out.stderr


def test_direct_light_is_in_the_usage_line_and_takes_no_value():
    assert "[--light KEY=R,G,B]... [--direct-light]" in run("--help").stdout
    assert run("--list").stdout == run("--list", "--light", "lamp=1", "--direct-light").stdout  # the registry's list, unchanged


@pytest.mark.gpu
@pytest.mark.parametrize("renderer,sm", [("hip_ray_tracer", False), ("hip_sm", True)])
def test_the_plugin_renders_the_restatements_frame(tmp_path, renderer, sm):
    from tests import direct_reference as direct_ref
    from tests import light_reference as light_ref

    ppm = tmp_path / "frame.ppm"
    out = run("--renderer", renderer, "--scene", LIGHTS, "--size", "96x54", "--spp", "20", "--seed", "11", "--light", "lamp=4,3.2,2", "--direct-light", "--out", str(ppm))
    assert out.returncode == 0 and "error:" not in out.stderr, out.stderr
    header = b"P6\n96 54\n255\n"
    got = np.frombuffer(ppm.read_bytes()[len(header) :], dtype=np.uint8).reshape(54, 96, 3)
    pod = light_ref.lights_scene(spp=20).describe(96, 54)
    want, _, _ = direct_ref.render(pod, 96, 54, light_ref.LIGHTS_TABLE, seed=11, want_rgb=False, sm_materials=sm)
    assert np.array_equal(got, unpack(want)[..., :3])
    implicit, _, _ = light_ref.render(pod, 96, 54, light_ref.LIGHTS_TABLE, seed=11, want_rgb=False, sm_materials=sm)
    assert not np.array_equal(want, implicit)  # (the flag reached the frame)
