"""rt_headless --bloom SPEC (rt_amd/host/main.cpp): what it refuses before it renders, by name — no GPU — and, on one, that the file it
writes is the frame the binding's render_bloomed gives, with --tonemap's curve and, without one, with the plain finish."""
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
    assert out.returncode == 0 and "[--bloom SPEC]" in out.stdout


@pytest.mark.parametrize("option", [("--progressive", "16"), ("--temporal",), ("--adaptive", "0.05"), ("--upscale", "2"), ("--progressive", "16", "--denoise")])
@pytest.mark.parametrize("first", [True, False])
def test_bloom_is_refused_with_every_frame_mode_by_name(option, first):
    bloom = ("--bloom", "default")
    args = (*bloom, *option) if first else (*option, *bloom)
    out = run("--renderer", "hip", "--scene", "basic.toml", *args)
    assert out.returncode == 2 and "error: --bloom blooms one-shot frames of a hip tracer" in out.stderr and f"refused with {option[0]}\n" in out.stderr
    assert "created renderer" not in out.stdout  # refused before anything is created


@pytest.mark.parametrize("renderer", ["null_renderer", "hip_rasterizer"])
def test_bloom_needs_a_hip_tracer(renderer):
    out = run("--renderer", renderer, "--scene", "basic.toml", "--bloom", "intensity=0.5")
    assert out.returncode == 2 and f"not '{renderer}'" in out.stderr and "refused with this renderer" in out.stderr


@pytest.mark.parametrize("spec", ["glow", "intensity=", "intensity=-1", "levels=9", "knee=2", "intensity=0.1;knee=0.2", ""])
def test_an_unreadable_spec_is_refused_with_the_parsers_words(spec):
    out = run("--renderer", "hip", "--scene", "basic.toml", "--bloom", spec)
    assert out.returncode == 2 and "error: --bloom expects default or KEY=VALUE items" in out.stderr and "rt_hip_bloom_from_spec: '" + spec in out.stderr


def test_a_missing_value_is_said():
    out = run("--bloom")
    assert out.returncode == 2 and "missing value for --bloom" in out.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("tonemap", [None, "aces"])
def test_rt_headless_bloom_writes_the_frame_the_binding_gives(tracer, tmp_path, tonemap):
    from rt_amd import capi, renderer
    from tests import light_reference as light_ref
    from tests.conftest import unpack

    ppm = tmp_path / "frame.ppm"
    curve = ("--tonemap", tonemap) if tonemap else ()
    out = run("--renderer", "hip", "--scene", LIGHTS_SCENE, "--size", "64x36", "--spp", "20", "--seed", "11", "--light", "lamp=4,3.2,2", "--bloom", "intensity=0.5,levels=8", *curve, "--out", str(ppm))
    assert out.returncode == 0 and "error:" not in out.stderr, out.stderr
    header = b"P6\n64 36\n255\n"
    got = np.frombuffer(ppm.read_bytes()[len(header) :], dtype=np.uint8).reshape(36, 64, 3)

    pod = light_ref.lights_scene(spp=20).describe(64, 36)
    try:
        tracer.set_emission(light_ref.LIGHTS_TABLE)
        want, _, _, _ = tracer.render_bloomed(pod, 64, 36, seed=11, flags=capi.RT_HIP_FLAG_EMISSION, bloom_params=renderer.bloom_from_spec("intensity=0.5,levels=8"),
                                              tonemap_params=renderer.tonemap_from_spec(tonemap or "none:1"))
        plain, _, _ = tracer.render(pod, 64, 36, seed=11, flags=capi.RT_HIP_FLAG_EMISSION)
    finally:
        tracer.set_emission(None)  # (the session's context is shared: no other test file sees a table)
    assert np.array_equal(got, unpack(want)[..., :3])
    assert not np.array_equal(want, plain)
