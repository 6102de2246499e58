"""rt_headless --lens aperture=A,focus=F (rt_amd/host/main.cpp): what it refuses before it renders, by name — no GPU — and, on one, that
the file it writes is the frame the CPU restatement of the lens contract gives (tests/native/lens_reference.cpp)."""
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT

BIN = ROOT / "rt_amd" / "bin" / "rt_headless"
SPEC = "aperture=0.06,focus=3.4"


def run(*args, **kw):
    return subprocess.run([str(BIN), *args], cwd=ROOT, capture_output=True, text=True, timeout=300, **kw)


def test_the_option_is_in_the_usage_line():
    out = run("--help")
    assert out.returncode == 0 and "[--lens aperture=A,focus=F]" in out.stdout


@pytest.mark.parametrize("option", [("--progressive", "16"), ("--adaptive", "0.05"), ("--temporal",), ("--progressive", "16", "--denoise"), ("--upscale", "2"), ("--boxes",), ("--light", "0=1")])
@pytest.mark.parametrize("first", [True, False])
def test_lens_is_refused_with_every_other_kind_of_frame(option, first):
    lens = ("--lens", SPEC)
    args = (*lens, *option) if first else (*option, *lens)
    out = run("--renderer", "hip", "--scene", "basic.toml", *args)
    assert out.returncode == 2 and "error: --lens takes one-shot frames of a hip renderer through a thin lens" in out.stderr
    assert "--progressive, --adaptive, --temporal, --denoise, --upscale, --boxes or --light" in out.stderr
    assert "created renderer" not in out.stdout  # refused before anything is created


def test_lens_needs_a_hip_renderer():
    out = run("--renderer", "null_renderer", "--scene", "basic.toml", "--lens", SPEC)
    assert out.returncode == 2 and "error: --lens takes one-shot frames of a hip renderer" in out.stderr and "not 'null_renderer'" in out.stderr


@pytest.mark.parametrize("spec", ["wide", "aperture=0.05", "aperture=-1,focus=2", "aperture=0.05,focus=0", "aperture=0.05;focus=1", ""])
def test_an_unreadable_spec_is_refused_with_the_parsers_words(spec):
    out = run("--renderer", "hip", "--scene", "basic.toml", "--lens", spec)
    assert out.returncode == 2 and "error: --lens expects aperture=A,focus=F" in out.stderr and "rt_hip_lens_from_spec: " in out.stderr


def test_a_missing_value_is_said():
    out = run("--lens")
    assert out.returncode == 2 and "missing value for --lens" in out.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("sm", [False, True])
def test_rt_headless_lens_writes_the_restatements_frame(tmp_path, sm):
    from tests import lens_reference as lens_ref
    from tests.conftest import unpack

    ppm = tmp_path / "frame.ppm"
    out = run("--renderer", "hip_sm" if sm else "hip", "--scene", "basic.toml", "--size", "64x36", "--spp", "20", "--seed", "11", "--lens", SPEC, "--out", str(ppm))
    assert out.returncode == 0 and "error:" not in out.stderr, out.stderr
    header = b"P6\n64 36\n255\n"
    got = np.frombuffer(ppm.read_bytes()[len(header) :], dtype=np.uint8).reshape(36, 64, 3)
    pod = lens_ref.named_scene("basic", None, 20).describe(64, 36)
    want, _, _ = lens_ref.render(pod, 64, 36, (0.06, 3.4), seed=11, want_rgb=False, sm_materials=sm)
    sharp, _, _ = lens_ref.render(pod, 64, 36, None, seed=11, want_rgb=False, sm_materials=sm)
    assert np.array_equal(got, unpack(want)[..., :3]) and not np.array_equal(want, sharp)
