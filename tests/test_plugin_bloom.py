"""RT_HIP_BLOOM in the hip_ray_tracer plug-in (shim/rt_hip_plugin.hpp), pinned on the CPU with the harness of tests/test_plugin_calls.py
— its sources exactly as they are, by g++ alone — built three times:

* as it is, and with tests/native/plugin_tonemap_fake.cpp: neither defines rt_hip_render_bloomed or rt_hip_bloom_from_spec, the plug-in
  declares both weak and finds them null — libraries that LACK the call (the second one has tone mapping);
* with tests/native/plugin_bloom_fake.cpp, which defines recording fakes of the two and brings the tone-mapping fakes along — a library
  that HAS it.

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
LACKS, HAS_TONEMAP, HAS_BLOOM = None, "plugin_tonemap_fake.cpp", "plugin_bloom_fake.cpp"
DEFAULT_BLOOM = "threshold:1,knee:0.5,intensity:0.1,scatter:0.7,levels:6"
PLAIN_FINISH = "curve:0,exposure:1,adaptation:1"  # none:1


@functools.lru_cache(maxsize=None)
def executable(fake):
    exe = tempfile.mkdtemp(prefix="plugin_bloom_") + "/plugin_calls"
    host = ROOT / "rt_amd" / "host"
    sources = [ROOT / "tests" / "native" / "plugin_calls.cpp", PLUGINS[1], host / "scene.cpp", host / "toml_subset.cpp"]
    if fake:
        sources.append(ROOT / "tests" / "native" / fake)
    command = [shutil.which("g++"), "-std=c++20", "-O1", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}", f"-I{host}", *map(str, sources), "-o", exe]
    built = subprocess.run(command, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    return exe


def run(fake, env, renderer="hip_ray_tracer", frames=3):
    """-> ([per frame: [(call, {field: text})]], the plug-in's stderr lines, the whole log)"""
    clean = {k: v for k, v in os.environ.items() if not k.startswith(("RT_HIP_", "PLUGIN_CALLS_"))}
    out = subprocess.run([executable(fake), renderer, str(frames)], env={**clean, **env}, cwd=ROOT, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and not out.stderr, (env, out.returncode, out.stderr)
    log, _, said = out.stdout.partition("stderr:\n")
    per_frame = []
    for line in log.splitlines():
        if line.startswith("frame "):
            per_frame.append([])
        elif per_frame:
            words = line.split(" ")
            per_frame[-1].append((words[0], dict(w.split("=", 1) for w in words[1:] if "=" in w)))
    return per_frame, said.splitlines(), out.stdout


def delivering(per_frame):
    """per frame, the calls that deliver a frame"""
    return [[(call, fields) for call, fields in frame if call.startswith("rt_hip_render")] for frame in per_frame[:3]]


def names(per_frame):
    return [[call for call, _ in frame] for frame in delivering(per_frame)]


@pytest.mark.parametrize("fake", [LACKS, HAS_TONEMAP])
def test_a_library_that_lacks_the_call_is_said_once_and_the_frames_are_as_before(fake):
    per_frame, said, _ = run(fake, {"RT_HIP_BLOOM": "default"})
    assert names(per_frame) == [["rt_hip_render"]] * 3
    assert said == ["error: hip_ray_tracer: RT_HIP_BLOOM is ignored: this librt_hip.so has no rt_hip_render_bloomed"]
    plain, nothing, _ = run(fake, {})
    assert delivering(per_frame) == delivering(plain) and nothing == []  # ... exactly the frames of a plug-in that was told nothing


def test_without_the_call_tone_mapped_frames_stay_tone_mapped():
    per_frame, said, _ = run(HAS_TONEMAP, {"RT_HIP_BLOOM": "intensity=0.5", "RT_HIP_TONEMAP": "reinhard:2"})
    without, _, _ = run(HAS_TONEMAP, {"RT_HIP_TONEMAP": "reinhard:2"})
    assert names(per_frame) == [["rt_hip_render_tonemapped"]] * 3 and delivering(per_frame) == delivering(without)
    assert said == ["error: hip_ray_tracer: RT_HIP_BLOOM is ignored: this librt_hip.so has no rt_hip_render_bloomed"]


def test_without_the_variable_the_log_is_byte_for_byte_the_same():
    """... whatever the library has: the plug-in asks nothing and says nothing about bloom (tests/test_plugin_calls.py holds the log of
    the library that lacks everything to tests/golden/plugin_calls.txt)."""
    for env in ({}, {"RT_HIP_BLOOM": ""}, {"RT_HIP_TONEMAP": "aces"}, {"RT_HIP_LIGHTS": "lamp=4", "RT_HIP_BLOOM": ""}):
        quiet = {k: v for k, v in env.items() if k != "RT_HIP_BLOOM"}
        assert run(HAS_BLOOM, env)[2] == run(HAS_TONEMAP, quiet)[2], env
        assert "bloom" not in run(HAS_BLOOM, env)[2]
    assert run(HAS_BLOOM, {})[2] == run(LACKS, {})[2]


@pytest.mark.parametrize("renderer", TRACERS)
@pytest.mark.parametrize("spec,bloom", [("default", DEFAULT_BLOOM), ("intensity=0.25", "threshold:1,knee:0.5,intensity:0.25,scatter:0.7,levels:6"),
                                        ("threshold=2,knee=1,scatter=1,levels=8,intensity=3", "threshold:2,knee:1,intensity:3,scatter:1,levels:8")])
def test_the_call_is_made_per_frame_with_the_parsed_parameters_and_the_plain_finish(renderer, spec, bloom):
    per_frame, said, _ = run(HAS_BLOOM, {"RT_HIP_BLOOM": spec}, renderer)
    assert said == []
    parses = [(call, fields) for frame in per_frame for call, fields in frame if call.endswith("_from_spec") and ("bloom" in call or "tonemap" in call)]
    assert parses == [("rt_hip_bloom_from_spec", {"spec": f"'{spec}'", "out_params": "set"}), ("rt_hip_tonemap_from_spec", {"spec": "'none:1'", "out_params": "set"})]  # each read once
    frames = delivering(per_frame)
    assert names(per_frame) == [["rt_hip_render_bloomed"]] * 3
    for number, ((_, fields),) in enumerate(frames, 1):
        assert fields["bloom"] == bloom and fields["tonemap"] == PLAIN_FINISH
        assert int(fields["seed"]) == number and int(fields["flags"], 16) == (FLAG_SM if renderer == "hip_sm_ray_tracer" else 0)
        assert (fields["ctx"], fields["scene"], fields["pixels"], fields["rgb_f32"], fields["stats"], fields["out_info"]) == ("set", "set", "set", "null", "null", "null")


@pytest.mark.parametrize("tonemap,curve", [("aces", "curve:2,exposure:0,adaptation:1"), ("reinhard:2", "curve:1,exposure:2,adaptation:1"), ("none:auto", "curve:0,exposure:0,adaptation:1")])
def test_with_rt_hip_tonemap_it_is_that_curve(tonemap, curve):
    per_frame, said, _ = run(HAS_BLOOM, {"RT_HIP_BLOOM": "default", "RT_HIP_TONEMAP": tonemap})
    assert said == [] and names(per_frame) == [["rt_hip_render_bloomed"]] * 3
    assert all(fields["tonemap"] == curve and fields["bloom"] == DEFAULT_BLOOM for ((_, fields),) in delivering(per_frame))
    parses = [fields["spec"] for frame in per_frame for call, fields in frame if call == "rt_hip_tonemap_from_spec"]
    assert parses == [f"'{tonemap}'"]  # (none:1 is not asked for)


def test_a_bad_tonemap_text_is_said_and_the_bloomed_frames_get_the_plain_finish():
    per_frame, said, _ = run(HAS_BLOOM, {"RT_HIP_BLOOM": "default", "RT_HIP_TONEMAP": "filmic"})
    assert names(per_frame) == [["rt_hip_render_bloomed"]] * 3 and all(fields["tonemap"] == PLAIN_FINISH for ((_, fields),) in delivering(per_frame))
    assert len(said) == 1 and said[0].endswith(": RT_HIP_TONEMAP is ignored")


def test_no_persistent_frame_flag_travels_and_lights_do():
    env = {"RT_HIP_BLOOM": "default", "RT_HIP_FRAME": "locked", "RT_HIP_LIGHTS": "lamp=4,3.2,2;0=0.5", "RT_HIP_DIRECT_LIGHT": "1", "RT_HIP_SEED": "5"}
    per_frame, said, _ = run(HAS_BLOOM, env)
    assert said == []
    for ((call, fields),) in delivering(per_frame):
        assert call == "rt_hip_render_bloomed" and int(fields["seed"]) == 5
        assert int(fields["flags"], 16) == FLAG_EMISSION | FLAG_DIRECT_LIGHT and not int(fields["flags"], 16) & FLAG_PERSISTENT_FRAME


@pytest.mark.parametrize("mode", list(MODES))
def test_a_frame_mode_makes_the_plugin_ignore_it_with_one_message(mode):
    per_frame, said, _ = run(HAS_BLOOM, {"RT_HIP_BLOOM": "default", mode: MODES[mode]})
    without, _, _ = run(HAS_BLOOM, {mode: MODES[mode]})
    assert delivering(per_frame) == delivering(without)  # the mode's own frames, untouched
    assert not any("bloom" in call or "tonemap" in call for frame in per_frame for call, _ in frame)
    assert said == [f"error: hip_ray_tracer: RT_HIP_BLOOM is ignored: {mode} is set, and only one-shot frames are bloomed"]


def test_the_rasterizer_ignores_it_with_one_message():
    per_frame, said, _ = run(HAS_BLOOM, {"RT_HIP_BLOOM": "default"}, "hip_rasterizer")
    without, _, _ = run(HAS_BLOOM, {}, "hip_rasterizer")
    assert delivering(per_frame) == delivering(without) and names(per_frame) == [["rt_hip_render"]] * 3
    assert said == ["error: hip_ray_tracer: RT_HIP_BLOOM is ignored: the preview has no float frame to bloom"]


@pytest.mark.parametrize("spec", ["glow", "intensity=-1", "intensity=", "levels=9", "knee=2", "Intensity=1"])
def test_a_bad_spec_is_ignored_with_the_quoted_message(spec):
    per_frame, said, _ = run(HAS_BLOOM, {"RT_HIP_BLOOM": spec})
    assert names(per_frame) == [["rt_hip_render"]] * 3
    assert len(said) == 1 and said[0].startswith("error: hip_ray_tracer: ") and said[0].endswith(": RT_HIP_BLOOM is ignored")
    assert f"message rt_hip_bloom_from_spec: '{spec}': " in run(HAS_BLOOM, {"RT_HIP_BLOOM": spec})[2]  # what the module leaves as its last error quotes the text
    # ... and with RT_HIP_TONEMAP the frames are the tone-mapped ones
    per_frame, said, _ = run(HAS_BLOOM, {"RT_HIP_BLOOM": spec, "RT_HIP_TONEMAP": "aces"})
    assert names(per_frame) == [["rt_hip_render_tonemapped"]] * 3 and len(said) == 1


def test_a_refusal_is_said_once_and_the_frames_fall_back():
    per_frame, said, _ = run(HAS_BLOOM, {"RT_HIP_BLOOM": "default", "PLUGIN_CALLS_UNSUPPORTED": "render_bloomed"})
    assert names(per_frame) == [["rt_hip_render_bloomed", "rt_hip_render"], ["rt_hip_render"], ["rt_hip_render"]]
    assert [int(fields["seed"]) for frame in delivering(per_frame) for _, fields in frame] == [1, 1, 2, 3]  # the refused frame keeps its seed
    assert len(said) == 1 and said[0].endswith(": RT_HIP_BLOOM is ignored for this renderer")
    per_frame, said, _ = run(HAS_BLOOM, {"RT_HIP_BLOOM": "default", "RT_HIP_TONEMAP": "aces", "PLUGIN_CALLS_UNSUPPORTED": "render_bloomed"})
    assert names(per_frame) == [["rt_hip_render_bloomed", "rt_hip_render_tonemapped"], ["rt_hip_render_tonemapped"], ["rt_hip_render_tonemapped"]]
    assert len(said) == 1 and said[0].endswith(": RT_HIP_BLOOM is ignored for this renderer")


def test_a_failure_is_said_every_frame_and_nothing_else_is_called():
    per_frame, said, _ = run(HAS_BLOOM, {"RT_HIP_BLOOM": "default", "PLUGIN_CALLS_FAIL": "render_bloomed"})
    assert names(per_frame) == [["rt_hip_render_bloomed"]] * 3
    assert len(said) == 3
