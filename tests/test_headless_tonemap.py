"""rt_headless --tonemap CURVE[:EXPOSURE] (rt_amd/host/main.cpp): what it refuses before it renders, by name — no GPU — and, on one,
that the file it writes is the frame the binding's render_tonemapped gives."""
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT

BIN = ROOT / "rt_amd" / "bin" / "rt_headless"
LIGHTS_SCENE = "tests/golden/scenes/lights.toml"


def run(*args, **kw):
    return subprocess.run([str(BIN), *args], cwd=ROOT, capture_output=True, text=True, timeout=300, **kw)


def test_the_option_is_in_the_usage_line():
    out = run("--help")
    assert out.returncode == 0 and "[--tonemap CURVE[:EXPOSURE]]" in out.stdout


@pytest.mark.parametrize("option", [("--progressive", "16"), ("--temporal",), ("--adaptive", "0.05"), ("--upscale", "2")])
@pytest.mark.parametrize("first", [True, False])
def test_tonemap_is_refused_with_every_frame_mode_by_name(option, first):
    tonemap = ("--tonemap", "aces")
    args = (*tonemap, *option) if first else (*option, *tonemap)
    out = run("--renderer", "hip", "--scene", "basic.toml", *args)
    assert out.returncode == 2 and f"error: --tonemap maps one-shot frames of a hip tracer" in out.stderr and f"refused with {option[0]}\n" in out.stderr
    assert "created renderer" not in out.stdout  # refused before anything is created


@pytest.mark.parametrize("renderer", ["null_renderer", "hip_rasterizer"])
def test_tonemap_needs_a_hip_tracer(renderer):
    out = run("--renderer", renderer, "--scene", "basic.toml", "--tonemap", "reinhard:2")
    assert out.returncode == 2 and f"not '{renderer}'" in out.stderr and "refused with this renderer" in out.stderr


@pytest.mark.parametrize("spec", ["filmic", "aces:", "aces:-1", "aces:0", "ACES", "reinhard:auto:1", ""])
def test_an_unreadable_spec_is_refused_with_the_parsers_words(spec):
    out = run("--renderer", "hip", "--scene", "basic.toml", "--tonemap", spec)
    assert out.returncode == 2 and "error: --tonemap expects CURVE[:EXPOSURE]" in out.stderr and "rt_hip_tonemap_from_spec: '" + spec in out.stderr


def test_a_missing_value_is_said():
    out = run("--tonemap")
    assert out.returncode == 2 and "missing value for --tonemap" in out.stderr


@pytest.mark.gpu
def test_rt_headless_tonemap_writes_the_frame_the_binding_gives(tracer, tmp_path):
    from rt_amd import capi, renderer
    from tests import light_reference as light_ref
    from tests.conftest import unpack

    ppm = tmp_path / "frame.ppm"
    out = run("--renderer", "hip", "--scene", LIGHTS_SCENE, "--size", "64x36", "--spp", "20", "--seed", "11", "--light", "lamp=4,3.2,2", "--tonemap", "aces", "--out", str(ppm))
    assert out.returncode == 0 and "error:" not in out.stderr, out.stderr
    header = b"P6\n64 36\n255\n"
    got = np.frombuffer(ppm.read_bytes()[len(header) :], dtype=np.uint8).reshape(36, 64, 3)

    pod = light_ref.lights_scene(spp=20).describe(64, 36)
    try:
        tracer.set_emission(light_ref.LIGHTS_TABLE)
        want, _, _, info = tracer.render_tonemapped(pod, 64, 36, seed=11, flags=capi.RT_HIP_FLAG_EMISSION, params=renderer.tonemap_from_spec("aces"))
        plain, _, _ = tracer.render(pod, 64, 36, seed=11, flags=capi.RT_HIP_FLAG_EMISSION)
    finally:
        tracer.set_emission(None)  # (the session's context is shared: no other test file sees a table)
    assert np.array_equal(got, unpack(want)[..., :3])
    assert info["counted"] == 64 * 36 and not np.array_equal(want, plain)
