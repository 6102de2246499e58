"""RT_HIP_TONEMAP in the hip_ray_tracer plug-in (shim/rt_hip_plugin.hpp), pinned on the CPU with the harness of tests/test_plugin_calls.py
— its sources exactly as they are, by g++ alone — built twice:

* as it is: the fake of tests/native/plugin_calls.cpp does not define rt_hip_render_tonemapped or rt_hip_tonemap_from_spec, the plug-in
  declares both weak and finds them null — a library that LACKS the call;
* with one more unit, tests/native/plugin_tonemap_fake.cpp, which defines recording fakes of the two — a library that HAS it.

One process per environment: the plug-in's getters are per-process statics."""
import functools
import os
import shutil
import subprocess
import tempfile

import pytest

from tests.conftest import ROOT
from tests.test_plugin_calls import MODES, PLUGINS, TRACERS

FLAG_PERSISTENT_FRAME, FLAG_EMISSION, FLAG_DIRECT_LIGHT, FLAG_SM = 1 << 2, 1 << 16, 1 << 17, 1 << 3
DEFAULTS = "low_permille:50,high_permille:20,exposure:{exposure},key:0.18,white:4,min_exposure:0.000976562,max_exposure:1024,adaptation:1"


@functools.lru_cache(maxsize=None)
def executable(with_the_call: bool):
    exe = tempfile.mkdtemp(prefix="plugin_tonemap_") + "/plugin_calls"
    host = ROOT / "rt_amd" / "host"
    sources = [ROOT / "tests" / "native" / "plugin_calls.cpp", PLUGINS[1], host / "scene.cpp", host / "toml_subset.cpp"]
    if with_the_call:
        sources.append(ROOT / "tests" / "native" / "plugin_tonemap_fake.cpp")
    command = [shutil.which("g++"), "-std=c++20", "-O1", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}", f"-I{host}", *map(str, sources), "-o", exe]
    built = subprocess.run(command, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    return exe


def run(with_the_call, env, renderer="hip_ray_tracer", frames=3):
    """-> ([per frame: [(call, {field: text})]], the plug-in's stderr lines)"""
    clean = {k: v for k, v in os.environ.items() if not k.startswith(("RT_HIP_", "PLUGIN_CALLS_"))}
    out = subprocess.run([executable(with_the_call), renderer, str(frames)], env={**clean, **env}, cwd=ROOT, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and not out.stderr, (env, out.returncode, out.stderr)
    log, _, said = out.stdout.partition("stderr:\n")
    per_frame = []
    for line in log.splitlines():
        if line.startswith("frame "):
            per_frame.append([])
        elif per_frame:
            words = line.split(" ")
            per_frame[-1].append((words[0], dict(w.split("=", 1) for w in words[1:] if "=" in w)))
    return per_frame, said.splitlines()


def delivering(per_frame):
    """per frame, the calls that deliver a frame"""
    return [[(call, fields) for call, fields in frame if call.startswith("rt_hip_render")] for frame in per_frame[:3]]


def test_a_library_that_lacks_the_call_is_said_once_and_the_frames_are_plain():
    per_frame, said = run(False, {"RT_HIP_TONEMAP": "aces"})
    assert [[call for call, _ in frame] for frame in delivering(per_frame)] == [["rt_hip_render"]] * 3
    assert said == ["error: hip_ray_tracer: RT_HIP_TONEMAP is ignored: this librt_hip.so has no rt_hip_render_tonemapped"]
    plain, nothing = run(False, {})
    assert delivering(per_frame) == delivering(plain) and nothing == []  # ... exactly the frames of a plug-in that was told nothing


@pytest.mark.parametrize("renderer", TRACERS)
@pytest.mark.parametrize("spec,curve,exposure", [("aces", 2, "0"), ("reinhard:2", 1, "2"), ("none:auto", 0, "0"), ("aces:0.125", 2, "0.125")])
def test_the_call_is_made_per_frame_with_the_parsed_parameters(renderer, spec, curve, exposure):
    per_frame, said = run(True, {"RT_HIP_TONEMAP": spec}, renderer)
    assert said == []
    parses = [fields for frame in per_frame for call, fields in frame if call == "rt_hip_tonemap_from_spec"]
    assert parses == [{"spec": f"'{spec}'", "out_params": "set"}]  # read once
    frames = delivering(per_frame)
    assert [[call for call, _ in frame] for frame in frames] == [["rt_hip_render_tonemapped"]] * 3
    for number, ((_, fields),) in enumerate(frames, 1):
        assert fields["params"] == f"curve:{curve}," + DEFAULTS.format(exposure=exposure)
        assert int(fields["seed"]) == number and int(fields["flags"], 16) == (FLAG_SM if renderer == "hip_sm_ray_tracer" else 0)
        assert (fields["ctx"], fields["scene"], fields["pixels"], fields["rgb_f32"], fields["stats"], fields["out_info"]) == ("set", "set", "set", "null", "null", "null")


def test_no_persistent_frame_flag_travels_and_lights_do():
    env = {"RT_HIP_TONEMAP": "aces", "RT_HIP_FRAME": "locked", "RT_HIP_LIGHTS": "lamp=4,3.2,2;0=0.5", "RT_HIP_DIRECT_LIGHT": "1", "RT_HIP_SEED": "5"}
    per_frame, said = run(True, env)
    assert said == []
    for ((call, fields),) in delivering(per_frame):
        assert call == "rt_hip_render_tonemapped" and int(fields["seed"]) == 5
        assert int(fields["flags"], 16) == FLAG_EMISSION | FLAG_DIRECT_LIGHT and not int(fields["flags"], 16) & FLAG_PERSISTENT_FRAME
    # ... while the plain frames of the same environment carry it
    per_frame, _ = run(True, {k: v for k, v in env.items() if k != "RT_HIP_TONEMAP"})
    assert all(int(fields["flags"], 16) & FLAG_PERSISTENT_FRAME for ((_, fields),) in delivering(per_frame))


@pytest.mark.parametrize("mode", list(MODES))
def test_a_frame_mode_makes_the_plugin_ignore_it_with_one_message(mode):
    args = {"RT_HIP_TONEMAP": "aces", mode: MODES[mode]}
    per_frame, said = run(True, args)
    without, _ = run(True, {mode: MODES[mode]})
    assert delivering(per_frame) == delivering(without)  # the mode's own frames, untouched
    assert not any(call.startswith("rt_hip_tonemap") or call == "rt_hip_render_tonemapped" for frame in per_frame for call, _ in frame)
    assert said == [f"error: hip_ray_tracer: RT_HIP_TONEMAP is ignored: {mode} is set, and only one-shot frames are tone-mapped"]


def test_the_rasterizer_ignores_it_with_one_message():
    per_frame, said = run(True, {"RT_HIP_TONEMAP": "aces"}, "hip_rasterizer")
    without, _ = run(True, {}, "hip_rasterizer")
    assert delivering(per_frame) == delivering(without) and [[call for call, _ in frame] for frame in delivering(per_frame)] == [["rt_hip_render"]] * 3
    assert said == ["error: hip_ray_tracer: RT_HIP_TONEMAP is ignored: the preview has no float frame to map"]


@pytest.mark.parametrize("spec", ["filmic", "aces:-1", "aces:", "ACES"])
def test_a_bad_spec_gets_one_message_and_plain_frames_follow(spec):
    per_frame, said = run(True, {"RT_HIP_TONEMAP": spec})
    assert [[call for call, _ in frame] for frame in delivering(per_frame)] == [["rt_hip_render"]] * 3
    assert len(said) == 1 and said[0].startswith("error: hip_ray_tracer: ") and said[0].endswith(": RT_HIP_TONEMAP is ignored")


def test_a_refusal_is_said_once_and_plain_frames_follow():
    per_frame, said = run(True, {"RT_HIP_TONEMAP": "aces", "PLUGIN_CALLS_UNSUPPORTED": "render_tonemapped"})
    assert [[call for call, _ in frame] for frame in delivering(per_frame)] == [["rt_hip_render_tonemapped", "rt_hip_render"], ["rt_hip_render"], ["rt_hip_render"]]
    assert [int(fields["seed"]) for frame in delivering(per_frame) for _, fields in frame] == [1, 1, 2, 3]  # the refused frame keeps its seed
    assert len(said) == 1 and said[0].endswith(": RT_HIP_TONEMAP is ignored for this renderer")


def test_a_failure_is_said_every_frame_and_nothing_else_is_called():
    per_frame, said = run(True, {"RT_HIP_TONEMAP": "aces", "PLUGIN_CALLS_FAIL": "render_tonemapped"})
    assert [[call for call, _ in frame] for frame in delivering(per_frame)] == [["rt_hip_render_tonemapped"]] * 3
    assert len(said) == 3


def test_unset_or_empty_says_nothing_and_asks_nothing():
    for env in ({}, {"RT_HIP_TONEMAP": ""}):
        per_frame, said = run(True, env)
        assert said == [] and [[call for call, _ in frame] for frame in delivering(per_frame)] == [["rt_hip_render"]] * 3
        assert not any("tonemap" in call for frame in per_frame for call, _ in frame)
