"""rt_headless --upscale (rt_amd/host/main.cpp): the option's argument checks, by name, without a GPU.  (The frame the
plug-in renders from RT_HIP_UPSCALE is held to the drop-in call in tests/test_gpu_upsample.py.)"""
import subprocess

import pytest

from tests.conftest import ROOT

BIN = ROOT / "rt_amd" / "bin" / "rt_headless"
MESSAGE = "--upscale traces one-shot frames of a hip renderer at 1 / FACTOR of the size and rebuilds them (not with --progressive, --temporal, --adaptive, --light or --box-bvh, not '"


def run(*args, **kw):
    return subprocess.run([str(BIN), *args], cwd=ROOT, capture_output=True, text=True, timeout=300, **kw)


@pytest.mark.parametrize("other,name", [(("--progressive", "16"), "--progressive"), (("--temporal",), "--temporal"), (("--adaptive", "0.03"), "--adaptive"), (("--light", "lamp=4,3.2,2"), "--light"),
                                        (("--progressive", "16", "--denoise"), "--progressive"), (("--temporal", "--denoise"), "--temporal"), (("--boxes", "--box-bvh"), "--box-bvh")])
def test_upscale_is_refused_with_the_options_it_does_not_compose_with_by_name(other, name):
    out = run("--upscale", "2", *other, "--renderer", "hip", "--scene", "basic.toml", "--size", "16x8")
    assert out.returncode == 2 and ("error: " + MESSAGE + "hip_ray_tracer'): refused with " + name) in out.stderr, out.stderr
    assert "created renderer" not in out.stdout  # nothing was created, nothing rendered


def test_upscale_is_refused_for_a_renderer_that_is_not_a_hip_one():
    out = run("--upscale", "2", "--renderer", "null", "--scene", "basic.toml", "--size", "16x8")
    assert out.returncode == 2 and ("error: " + MESSAGE + "null_renderer')") in out.stderr, out.stderr


@pytest.mark.parametrize("factor", ["0", "1", "5", "two", "2x", "-2", ""])
def test_upscale_expects_a_factor_of_2_to_4(factor):
    out = run("--upscale", factor, "--renderer", "hip", "--scene", "basic.toml")
    assert out.returncode == 2 and "--upscale expects the factor (2, 3 or 4)" in out.stderr, out.stderr


def test_upscale_needs_a_value_and_is_in_the_usage_line():
    out = run("--upscale")
    assert out.returncode == 2 and "missing value for --upscale" in out.stderr
    assert "[--upscale FACTOR]" in run("--help").stdout
    assert run("--list").stdout == run("--list", "--upscale", "2").stdout  # the registry's list, unchanged


def test_denoise_alone_still_needs_progressive_and_composes_with_upscale():
    out = run("--scene", "basic.toml", "--denoise")
    assert out.returncode == 2 and "--denoise" in out.stderr and "--progressive" in out.stderr
    # with --upscale the pair passes the argument checks: what stops this run is the renderer that is no hip one
    out = run("--upscale", "3", "--denoise", "--renderer", "null", "--scene", "basic.toml")
    assert out.returncode == 2 and MESSAGE in out.stderr and "--denoise filters" not in out.stderr
