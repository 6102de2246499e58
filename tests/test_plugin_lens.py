"""RT_HIP_LENS in the hip_ray_tracer plug-in (shim/rt_hip_plugin.hpp), pinned on the CPU with the harness of
tests/test_plugin_calls.py — its sources exactly as they are, by g++ alone — built with and without the two entry points:

* as it is, and with tests/native/plugin_bloom_fake.cpp: neither defines rt_hip_set_lens or rt_hip_lens_from_spec, the plug-in declares
  both weak and finds them null — libraries that LACK the calls (the second one has bloom and tone mapping);
* with tests/native/plugin_lens_fake.cpp, which defines recording fakes of the two and brings the older fakes along — a library that HAS
  them.

One process per environment: the plug-in's getters are per-process statics."""
import pytest

from tests.test_plugin_bloom import delivering, names, run
from tests.test_plugin_calls import MODES, TRACERS

FLAG_PERSISTENT_FRAME, FLAG_SM, FLAG_THIN_LENS = 1 << 2, 1 << 3, 1 << 18
LACKS, HAS_BLOOM, HAS_LENS = None, "plugin_bloom_fake.cpp", "plugin_lens_fake.cpp"
SPEC = "aperture=0.05,focus=4.2"


def lens_calls(per_frame):
    return [(call, fields) for frame in per_frame for call, fields in frame if "lens" in call]


@pytest.mark.parametrize("fake", [LACKS, HAS_BLOOM])
def test_a_library_that_lacks_the_calls_is_said_once_and_the_frames_are_as_before(fake):
    per_frame, said, _ = run(fake, {"RT_HIP_LENS": SPEC})
    assert names(per_frame) == [["rt_hip_render"]] * 3
    assert said == ["error: hip_ray_tracer: RT_HIP_LENS is ignored: this librt_hip.so has no rt_hip_set_lens"]
    plain, nothing, _ = run(fake, {})
    assert delivering(per_frame) == delivering(plain) and nothing == []  # ... exactly the frames of a plug-in that was told nothing


def test_without_the_variable_the_log_is_byte_for_byte_the_same():
    """... whatever the library has: the plug-in asks nothing and says nothing about a lens (tests/test_plugin_calls.py holds the log of
    the library that lacks everything to tests/golden/plugin_calls.txt)."""
    for env in ({}, {"RT_HIP_LENS": ""}, {"RT_HIP_TONEMAP": "aces"}, {"RT_HIP_LIGHTS": "lamp=4", "RT_HIP_BLOOM": "default"}):
        quiet = {k: v for k, v in env.items() if k != "RT_HIP_LENS"}
        assert run(HAS_LENS, env)[2] == run(HAS_BLOOM, quiet)[2], env
        assert "lens" not in run(HAS_LENS, env)[2]
    assert run(HAS_LENS, {})[2] == run(LACKS, {})[2]


@pytest.mark.parametrize("renderer", TRACERS)
def test_the_lens_is_set_once_and_every_frame_carries_the_flag(renderer):
    per_frame, said, _ = run(HAS_LENS, {"RT_HIP_LENS": SPEC}, renderer)
    assert said == []
    assert lens_calls(per_frame) == [("rt_hip_lens_from_spec", {"spec": f"'{SPEC}'", "out_lens": "set"}), ("rt_hip_set_lens", {"ctx": "set", "lens": "aperture:0.05,focus:4.2"})]  # each once, in this order
    assert [call for call, _ in per_frame[0]].index("rt_hip_set_lens") < [call for call, _ in per_frame[0]].index("rt_hip_render")  # in front of the first frame
    assert names(per_frame) == [["rt_hip_render"]] * 3
    for number, ((_, fields),) in enumerate(delivering(per_frame), 1):
        assert int(fields["seed"]) == number and int(fields["flags"], 16) == FLAG_THIN_LENS | (FLAG_SM if renderer == "hip_sm_ray_tracer" else 0)


def test_it_composes_with_tone_mapping_and_bloom_and_the_frame_flag():
    per_frame, said, _ = run(HAS_LENS, {"RT_HIP_LENS": SPEC, "RT_HIP_TONEMAP": "aces"})
    assert said == [] and names(per_frame) == [["rt_hip_render_tonemapped"]] * 3
    assert all(int(fields["flags"], 16) == FLAG_THIN_LENS for ((_, fields),) in delivering(per_frame))
    per_frame, said, _ = run(HAS_LENS, {"RT_HIP_LENS": SPEC, "RT_HIP_TONEMAP": "aces", "RT_HIP_BLOOM": "default"})
    assert said == [] and names(per_frame) == [["rt_hip_render_bloomed"]] * 3
    assert all(int(fields["flags"], 16) == FLAG_THIN_LENS for ((_, fields),) in delivering(per_frame))
    per_frame, said, _ = run(HAS_LENS, {"RT_HIP_LENS": SPEC, "RT_HIP_FRAME": "locked"})
    assert said == [] and all(int(fields["flags"], 16) == FLAG_THIN_LENS | FLAG_PERSISTENT_FRAME for ((_, fields),) in delivering(per_frame))
    # a bloomed frame the module refuses falls back to the plain one, which keeps the lens
    per_frame, said, _ = run(HAS_LENS, {"RT_HIP_LENS": SPEC, "RT_HIP_BLOOM": "default", "PLUGIN_CALLS_UNSUPPORTED": "render_bloomed"})
    assert names(per_frame) == [["rt_hip_render_bloomed", "rt_hip_render"], ["rt_hip_render"], ["rt_hip_render"]] and len(said) == 1
    assert all(int(fields["flags"], 16) == FLAG_THIN_LENS for frame in delivering(per_frame) for _, fields in frame)


@pytest.mark.parametrize("other,value", [*MODES.items(), ("RT_HIP_LIGHTS", "lamp=4,3.2,2")])
def test_a_frame_mode_or_lights_make_the_plugin_ignore_it_with_one_message(other, value):
    per_frame, said, _ = run(HAS_LENS, {"RT_HIP_LENS": SPEC, other: value})
    without, _, _ = run(HAS_LENS, {other: value})
    assert delivering(per_frame) == delivering(without)  # the other variable's own frames, untouched
    assert lens_calls(per_frame) == []
    assert said == [f"error: hip_ray_tracer: RT_HIP_LENS is ignored: {other} is set, and only one-shot frames without lights are taken through a lens"]


def test_the_rasterizer_ignores_it_without_a_word():
    per_frame, said, _ = run(HAS_LENS, {"RT_HIP_LENS": SPEC}, "hip_rasterizer")
    without, _, _ = run(HAS_LENS, {}, "hip_rasterizer")
    assert delivering(per_frame) == delivering(without) and lens_calls(per_frame) == [] and said == []


@pytest.mark.parametrize("spec", ["wide", "aperture=0.05", "aperture=-1,focus=2", "aperture=0.05,focus=0", "aperture=0.05,focus=4.2,blades=6"])
def test_a_bad_spec_is_ignored_with_the_message(spec):
    per_frame, said, log = run(HAS_LENS, {"RT_HIP_LENS": spec})
    assert names(per_frame) == [["rt_hip_render"]] * 3 and all(int(fields["flags"], 16) == 0 for ((_, fields),) in delivering(per_frame))
    assert [call for call, _ in lens_calls(per_frame)] == ["rt_hip_lens_from_spec"]  # asked once, nothing set
    assert len(said) == 1 and said[0].startswith("error: hip_ray_tracer: ") and said[0].endswith(": RT_HIP_LENS is ignored")
    assert "message rt_hip_lens_from_spec: " in log


def test_a_lens_the_module_refuses_is_said_once_and_the_frames_are_the_pinholes():
    per_frame, said, _ = run(HAS_LENS, {"RT_HIP_LENS": SPEC, "PLUGIN_CALLS_FAIL": "set_lens"})
    assert names(per_frame) == [["rt_hip_render"]] * 3 and all(int(fields["flags"], 16) == 0 for ((_, fields),) in delivering(per_frame))
    assert [call for call, _ in lens_calls(per_frame)] == ["rt_hip_lens_from_spec", "rt_hip_set_lens"]
    assert len(said) == 1 and said[0].endswith(": RT_HIP_LENS is ignored")
