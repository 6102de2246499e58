"""What the hip_ray_tracer plug-in asks of the module, pinned on the CPU (no GPU, nothing of ROCm).

tests/native/plugin_calls.cpp links the mirror plug-in (rt_amd/host/hip_ray_tracer.cpp, whose body is shim/rt_hip_plugin.hpp — the
very text the uncompilable shim instantiates) against a recording fake of the sixteen C entry points it uses.  One process per
environment, because the plug-in's getters are per-process statics.

tests/golden/plugin_calls.txt is the behaviour of the plug-in as it stood BEFORE its body was written once: it was recorded with this
harness built against that commit's rt_amd/host/hip_ray_tracer.cpp

    git show <that commit>:rt_amd/host/hip_ray_tracer.cpp > <dir>/hip_ray_tracer.cpp
    python -m tests.test_plugin_calls record <dir>/hip_ray_tracer.cpp > tests/golden/plugin_calls.txt

and is never written from the code under test: a change of the plug-in's behaviour is made here by hand, line by line, or recorded
from a plug-in source that is known good.  `python -m tests.test_plugin_calls check PROGRAM VARIABLE...` holds an already built
harness (`make sanitize-plugin`: the one under AddressSanitizer and UndefinedBehaviorSanitizer) to the rows that set one of the
variables."""
import functools
import itertools
import os
import shutil
import subprocess
import sys
import tempfile

import pytest

from tests.conftest import ROOT

GOLDEN = ROOT / "tests" / "golden" / "plugin_calls.txt"
PLUGINS = [ROOT / "shim" / "hip_ray_tracer.cpp", ROOT / "rt_amd" / "host" / "hip_ray_tracer.cpp"]
MARKER = "// ---- from here on shim/hip_ray_tracer.cpp and rt_amd/host/hip_ray_tracer.cpp are one text"
TRACERS = ("hip_ray_tracer", "hip_sm_ray_tracer")
RENDERERS = (*TRACERS, "hip_rasterizer")
FLAG_PERSISTENT_FRAME = 1 << 2
ACCUMULATING = ("rt_hip_render_progressive", "rt_hip_render_adaptive", "rt_hip_render_temporal", "rt_hip_render_upscaled")
# (the order render() asks in, and what each is set to where the matrix sets it)
MODES = {"RT_HIP_ADAPTIVE": "0.05", "RT_HIP_TEMPORAL": "1", "RT_HIP_PROGRESSIVE": "2", "RT_HIP_UPSCALE": "2"}
MODE_CALL = dict(zip(MODES, ("rt_hip_render_adaptive", "rt_hip_render_temporal", "rt_hip_render_progressive", "rt_hip_render_upscaled")))
LIGHTS = "lamp=4,3.2,2;0=0.5"


def _matrix():
    """(id, renderer, frames, arguments, environment) of every run; the id is the golden file's section title."""
    rows = []

    def row(env, renderer="hip_ray_tracer", frames=3, args=(), name=None):
        words = [renderer, *args, *(f"{k}={v}" for k, v in env.items())] if name is None else [renderer, name]
        rows.append((" ".join(words), renderer, frames, tuple(args), dict(env)))

    # plain frames
    for renderer in RENDERERS:
        for env in ({}, {"RT_HIP_SEED": "5"}, {"RT_HIP_FRAME": "locked"}):
            row(env, renderer)
    boxes = {"RT_HIP_TRACE_BOXES": "1", "RT_HIP_BOX_BVH": "1"}
    for accel in (None, "bvh", "bvh-device"):
        env = {} if accel is None else {"RT_HIP_ACCEL": accel}
        if accel:
            row(env)
        row({**env, **boxes})
    row({"RT_HIP_TRACE_BOXES": "1"})
    row({"RT_HIP_BOX_BVH": "1"})
    row({"RT_HIP_ACCEL": "bvh", **boxes}, "hip_rasterizer")
    # each frame mode alone
    for renderer in TRACERS:
        for denoise in (None, "1", "always"):
            row({"RT_HIP_PROGRESSIVE": "2", **({"RT_HIP_DENOISE": denoise} if denoise else {})}, renderer, args=("--spp", "5"))
        for denoise, seed in itertools.product((None, "1"), (None, "5")):
            row({"RT_HIP_TEMPORAL": "1", **({"RT_HIP_DENOISE": denoise} if denoise else {}), **({"RT_HIP_SEED": seed} if seed else {})}, renderer)
        for progressive in (None, "8", "40"):
            row({"RT_HIP_ADAPTIVE": "0.05", **({"RT_HIP_PROGRESSIVE": progressive} if progressive else {})}, renderer)
        for factor, denoise in itertools.product(("2", "4"), (None, "1")):
            row({"RT_HIP_UPSCALE": factor, **({"RT_HIP_DENOISE": denoise} if denoise else {})}, renderer)
    for mode, value in MODES.items():  # (what the rules below look at: a pinned seed and RT_HIP_FRAME=locked under every mode)
        row({mode: value, "RT_HIP_FRAME": "locked"})
        if mode in ("RT_HIP_ADAPTIVE", "RT_HIP_PROGRESSIVE"):
            row({mode: value, "RT_HIP_SEED": "5"})
    # precedence
    for renderer in ("hip_ray_tracer", "hip_rasterizer"):
        row(MODES, renderer)
        for pair in itertools.combinations(MODES, 2):
            row({mode: MODES[mode] for mode in pair}, renderer)
    # unreadable values
    for value in ("-1", "abc", "0.1x"):
        row({"RT_HIP_ADAPTIVE": value})
    for value in ("0", "1", "5", "2x"):
        row({"RT_HIP_UPSCALE": value})
    row({"RT_HIP_GROUP": "no_colons"})
    row({"RT_HIP_GROUP": "/" + "n" * 299 + ":0:2"}, name="RT_HIP_GROUP=<a name of 300 characters>:0:2")
    row({"RT_HIP_GROUP": "/rt_group:1:4"})
    row({"RT_HIP_GROUP": "/rt_group:1:4", "RT_HIP_DEVICE": "2"})
    row({"RT_HIP_GROUP": "/rt_group:1:4", "PLUGIN_CALLS_FAIL": "join_frame_group"})
    # contexts
    row({"RT_HIP_DEVICES": "all", "PLUGIN_CALLS_DEVICE_COUNT": "4"})
    row({"RT_HIP_DEVICES": "all", "PLUGIN_CALLS_DEVICE_COUNT": "0"})
    row({"RT_HIP_DEVICES": "0,1,2,3"})
    row({"RT_HIP_DEVICES": "2,"})
    row({"RT_HIP_DEVICES": "0,1", "RT_HIP_FRAME": "direct"})
    row({"RT_HIP_DEVICES": "0,1", "RT_HIP_FRAME": "locked+direct"})
    row({"RT_HIP_DEVICE": "3"})
    row({"PLUGIN_CALLS_CREATE_FAILS": "1"})
    # fall-backs
    for mode, value in MODES.items():
        call = MODE_CALL[mode][len("rt_hip_"):]
        if mode != "RT_HIP_PROGRESSIVE":  # (progressive passes have no "refused once": the module's message, every frame)
            row({mode: value, "PLUGIN_CALLS_UNSUPPORTED": call})
        row({mode: value, "PLUGIN_CALLS_FAIL": call})
    row({"RT_HIP_TEMPORAL": "1", "RT_HIP_SEED": "5", "PLUGIN_CALLS_UNSUPPORTED": "render_temporal"})
    row({"RT_HIP_TEMPORAL": "1", "PLUGIN_CALLS_UNSUPPORTED": "render_temporal", "PLUGIN_CALLS_FAIL": "render"})
    row({"RT_HIP_ADAPTIVE": "0.05", "RT_HIP_UPSCALE": "2", "PLUGIN_CALLS_UNSUPPORTED": "render_adaptive"})
    row({"RT_HIP_ADAPTIVE": "0.05", "RT_HIP_UPSCALE": "2", "PLUGIN_CALLS_UNSUPPORTED": "render_adaptive,render_upscaled"})
    row({"RT_HIP_PROGRESSIVE": "2", "RT_HIP_DENOISE": "always", "PLUGIN_CALLS_FAIL": "denoise_progressive"}, args=("--spp", "5"))
    row({"PLUGIN_CALLS_FAIL": "render"})
    # lights
    row({"RT_HIP_LIGHTS": LIGHTS})
    row({"RT_HIP_LIGHTS": LIGHTS}, "hip_sm_ray_tracer")
    row({"RT_HIP_LIGHTS": LIGHTS}, args=("--rename",))
    row({"RT_HIP_LIGHTS": LIGHTS, "PLUGIN_CALLS_FAIL": "set_emission"})
    row({"RT_HIP_LIGHTS": LIGHTS, "PLUGIN_CALLS_FAIL": "lights_from_spec"})
    row({"RT_HIP_LIGHTS": LIGHTS}, "hip_rasterizer")
    row({"RT_HIP_LIGHTS": LIGHTS, "RT_HIP_DIRECT_LIGHT": "1"})
    row({"RT_HIP_LIGHTS": LIGHTS, "RT_HIP_DIRECT_LIGHT": "0"})
    row({"RT_HIP_DIRECT_LIGHT": "1"})
    row({"RT_HIP_LIGHTS": ""})
    row({"RT_HIP_LIGHTS": LIGHTS, "RT_HIP_UPSCALE": "2", "PLUGIN_CALLS_UNSUPPORTED": "render_upscaled"})
    assert len({r[0] for r in rows}) == len(rows)
    return rows


MATRIX = _matrix()
BY_ID = {r[0]: r for r in MATRIX}


def build(plugin_source, flags=("-O1",), exe=None):
    """The harness with `plugin_source` as its plug-in, by g++ alone, warnings as errors."""
    exe = exe or tempfile.mkdtemp(prefix="plugin_calls_") + "/plugin_calls"
    host = ROOT / "rt_amd" / "host"
    sources = [ROOT / "tests" / "native" / "plugin_calls.cpp", plugin_source, host / "scene.cpp", host / "toml_subset.cpp"]
    command = [shutil.which("g++"), "-std=c++20", *flags, "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}", f"-I{host}", *map(str, sources), "-o", exe]
    built = subprocess.run(command, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    return exe


@functools.lru_cache(maxsize=None)
def executable():
    return build(PLUGINS[1])


def run(exe, case):
    """The call log and, behind it, what the plug-in said: the harness's stdout."""
    _, renderer, frames, args, env = BY_ID[case]
    clean = {k: v for k, v in os.environ.items() if not k.startswith(("RT_HIP_", "PLUGIN_CALLS_"))}
    out = subprocess.run([exe, renderer, str(frames), *args], env={**clean, **env}, cwd=ROOT, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and not out.stderr, (case, out.returncode, out.stderr)
    return out.stdout


@functools.lru_cache(maxsize=None)
def golden():
    sections = {}
    for line in GOLDEN.read_text().splitlines(keepends=True):
        if line.startswith("== "):
            title = line[3:].rstrip("\n")
            assert title not in sections
            sections[title] = ""
        else:
            sections[title] += line
    return sections


def test_the_golden_file_holds_the_matrix():
    assert list(golden()) == [r[0] for r in MATRIX]


@pytest.mark.parametrize("case", [r[0] for r in MATRIX])
def test_the_plugin_asks_what_it_asked_before(case):
    assert run(executable(), case) == golden()[case]


# ---- the rules a reader would look for, in plain words (over the recorded runs: the test above holds the plug-in to them) ----


def frames_of(case):
    """-> ([per frame: [(call, {field: text})]], the plug-in's stderr lines)"""
    log, _, said = golden()[case].partition("stderr:\n")
    frames = []
    for line in log.splitlines():
        if line.startswith("frame "):
            frames.append([])
        elif frames:  # (behind the last frame: rt_hip_destroy, which belongs to none)
            words = line.split(" ")
            frames[-1].append((words[0], dict(w.split("=", 1) for w in words[1:] if "=" in w)))
    return frames, said.splitlines()


def frame_calls(case):
    """per frame, the calls that deliver a frame (not the parameter getters, the table, the context)"""
    return [[(call, f) for call, f in frame if call == "rt_hip_render" or call in ACCUMULATING] for frame in frames_of(case)[0][:3]]


def case_of(env, renderer="hip_ray_tracer", args=()):
    return " ".join([renderer, *args, *(f"{k}={v}" for k, v in env.items())])


def test_precedence_adaptive_temporal_progressive_upscale_one_shot():
    """render() asks in that order and the first mode that is set takes the frame — with ONE exception that is the parent's own and
    stays: RT_HIP_TEMPORAL's getter gives way to RT_HIP_PROGRESSIVE ("is set and wins"), so of those two progressive takes it."""
    order = list(MODES)
    for n in (2, 4):
        for chosen in itertools.combinations(order, n):
            winner = chosen[0]
            if winner == "RT_HIP_TEMPORAL" and "RT_HIP_PROGRESSIVE" in chosen:
                winner = "RT_HIP_PROGRESSIVE"
            case = case_of({mode: MODES[mode] for mode in chosen})
            for frame in frame_calls(case):
                assert [call for call, _ in frame] == [MODE_CALL[winner]], case
            gave_way = [line for line in frames_of(case)[1] if "RT_HIP_TEMPORAL is ignored: RT_HIP_PROGRESSIVE is set and wins" in line]
            assert len(gave_way) == (1 if winner == "RT_HIP_PROGRESSIVE" and "RT_HIP_TEMPORAL" in chosen else 0), case
            # the preview takes none of them, and reaches no getter that could speak
            preview = case_of({mode: MODES[mode] for mode in chosen}, "hip_rasterizer")
            assert all([call for call, _ in frame] == ["rt_hip_render"] for frame in frame_calls(preview)) and frames_of(preview)[1] == []
    for mode in order:
        assert all([call for call, _ in frame] == [MODE_CALL[mode]] for frame in frame_calls(case_of({mode: MODES[mode], "RT_HIP_FRAME": "locked"})))
    assert all([call for call, _ in frame] == ["rt_hip_render"] for frame in frame_calls("hip_ray_tracer"))


def test_no_frame_flag_on_any_accumulating_call():
    seen = set()
    for case, *_, env in MATRIX:
        for frame in frames_of(case)[0]:
            for call, fields in frame:
                if call in ACCUMULATING:
                    seen.add(call)
                    assert int(fields["flags"], 16) & FLAG_PERSISTENT_FRAME == 0, case
                elif call == "rt_hip_render":  # (the one call that takes it, where it was asked for)
                    assert bool(int(fields["flags"], 16) & FLAG_PERSISTENT_FRAME) == ("locked" in env.get("RT_HIP_FRAME", "")), case
    assert seen == set(ACCUMULATING)


def test_seeds():
    """progressive and adaptive passes: 1 when unpinned, RT_HIP_SEED when pinned, the same for every pass (a seed per frame would
    start the accumulation again).  Temporal frames: the frame's number, RT_HIP_SEED + the frame's number when pinned.  One-shot and
    upscaled frames: the frame's number, or RT_HIP_SEED."""

    def seeds(env, args=()):
        return [int(fields["seed"]) for frame in frame_calls(case_of(env, args=args)) for _, fields in frame]

    assert seeds({"RT_HIP_PROGRESSIVE": "2"}, ("--spp", "5")) == [1, 1, 1] and seeds({"RT_HIP_PROGRESSIVE": "2", "RT_HIP_SEED": "5"}) == [5, 5, 5]
    assert seeds({"RT_HIP_ADAPTIVE": "0.05"}) == [1, 1, 1] and seeds({"RT_HIP_ADAPTIVE": "0.05", "RT_HIP_SEED": "5"}) == [5, 5, 5]
    assert seeds({"RT_HIP_TEMPORAL": "1"}) == [1, 2, 3] and seeds({"RT_HIP_TEMPORAL": "1", "RT_HIP_SEED": "5"}) == [6, 7, 8]
    assert seeds({}) == [1, 2, 3] and seeds({"RT_HIP_SEED": "5"}) == [5, 5, 5]
    assert seeds({"RT_HIP_UPSCALE": "2"}) == [1, 2, 3]
    # refused temporal frames keep the seed the frame got
    assert seeds({"RT_HIP_TEMPORAL": "1", "PLUGIN_CALLS_UNSUPPORTED": "render_temporal"}) == [1, 1, 2, 3]
    assert seeds({"RT_HIP_TEMPORAL": "1", "RT_HIP_SEED": "5", "PLUGIN_CALLS_UNSUPPORTED": "render_temporal"}) == [6, 6, 7, 8]


def test_min_samples_is_at_least_two_padded_passes():
    for progressive, pass_samples, min_samples in ((None, 16, 32), ("8", 8, 32), ("40", 40, 96)):
        case = case_of({"RT_HIP_ADAPTIVE": "0.05", **({"RT_HIP_PROGRESSIVE": progressive} if progressive else {})})
        for frame in frame_calls(case):
            ((_, fields),) = frame
            params = dict(item.split(":") for item in fields["params"].split(","))
            assert int(fields["pass_samples"]) == pass_samples and int(params["min_samples"]) == min_samples
            assert int(params["min_samples"]) >= 2 * ((pass_samples + 15) // 16 * 16)
            assert float(params["threshold"]) == pytest.approx(0.05, rel=1e-7) and float(params["floor"]) == pytest.approx(0.01, rel=1e-7)


@pytest.mark.parametrize("mode", ["RT_HIP_ADAPTIVE", "RT_HIP_TEMPORAL", "RT_HIP_UPSCALE"])
def test_a_refusal_is_said_once(mode):
    """RT_HIP_UNSUPPORTED from the mode's call: asked once, said once, and that frame and every later one is rt_hip_render's."""
    case = case_of({mode: MODES[mode], "PLUGIN_CALLS_UNSUPPORTED": MODE_CALL[mode][len("rt_hip_"):]})
    assert [[call for call, _ in frame] for frame in frame_calls(case)] == [[MODE_CALL[mode], "rt_hip_render"], ["rt_hip_render"], ["rt_hip_render"]]
    said = frames_of(case)[1]
    assert said == [f"error: hip_ray_tracer: fake {MODE_CALL[mode]} is unsupported: {mode} is ignored for this renderer"]


def test_the_two_plugin_files_are_one_text_below_the_marker():
    tails = []
    for path in PLUGINS:
        lines = path.read_text().splitlines()
        assert len(lines) <= 80, (path, len(lines))
        (at,) = [i for i, line in enumerate(lines) if line.startswith(MARKER)]
        tails.append(lines[at:])
        assert not any(line.startswith(("struct", "template", "REGISTER_RENDERER", "namespace", "using")) for line in map(str.strip, lines[:at])), path
    assert tails[0] == tails[1] and sum(line.strip().startswith("REGISTER_RENDERER(") for line in tails[0]) == 3


def _main(argv):
    if argv[:1] == ["record"] and len(argv) == 2:  # the matrix as the plug-in of argv[1] answers it: how the golden file was made
        exe = build(argv[1])
        sys.stdout.write("".join(f"== {case}\n{run(exe, case)}" for case, *_ in MATRIX))
        return 0
    if argv[:1] == ["check"] and len(argv) >= 3:  # an already built harness against the rows that set one of the variables
        cases = [case for case, *_, env in MATRIX if any(variable in env for variable in argv[2:])]
        wrong = [case for case in cases if run(argv[1], case) != golden()[case]]
        print(f"{len(cases)} runs of {argv[1]}, {len(wrong)} unlike tests/golden/plugin_calls.txt", *wrong, sep="\n")
        return 1 if wrong or not cases else 0
    print(__doc__)
    return 2


if __name__ == "__main__":
    sys.exit(_main(sys.argv[1:]))
