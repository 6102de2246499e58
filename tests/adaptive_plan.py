"""tests/native/adaptive_plan_dump.cpp, built once per test process: the host-only unit of adaptive sampling (defaults, parameter check,
sequencing, accepted flags, the launch plan of an adaptive pass) asked on the CPU.  Shared by tests/test_adaptive_host.py, which pins
the rules, and tests/test_gpu_adaptive.py, which asks it which tile shape — and so which fold path — an adaptive pass takes."""
import functools
import shutil
import struct
import subprocess
import tempfile

from tests.conftest import ROOT

SOURCES = [str(ROOT / "tests" / "native" / "adaptive_plan_dump.cpp")] + [str(ROOT / "rt_amd" / "csrc" / name) for name in ("adaptive.cpp", "launch_plan.cpp", "progressive.cpp")]


@functools.lru_cache(maxsize=None)
def executable():
    """The dump program, built with g++ alone (nothing of ROCm on the command line); None without a compiler."""
    cxx = shutil.which("g++")
    if cxx is None:
        return None
    exe = tempfile.mkdtemp(prefix="adaptive_plan_") + "/adaptive_plan_dump"
    built = subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", *SOURCES, "-o", exe], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    return exe


def ask(lines):
    """One answer line per command line."""
    out = subprocess.run([executable()], input="".join(line + "\n" for line in lines), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    answers = out.stdout.splitlines()
    assert len(answers) == len(lines)
    return answers


def word(value: float) -> int:
    return struct.unpack("<I", struct.pack("<f", value))[0]


def defaults():
    """-> (threshold, floor, min_samples)"""
    (line,) = ask(["defaults"])
    threshold, floor, min_samples = (int(v) for v in line.split())
    return struct.unpack("<f", struct.pack("<I", threshold))[0], struct.unpack("<f", struct.pack("<I", floor))[0], min_samples


def pass_size(pass_samples):
    return int(ask([f"size {pass_samples}"])[0])


def check(threshold, floor, min_samples, size=16):
    """-> (status, message or None); threshold and floor as floats or as raw words (ints)"""
    words = [v if isinstance(v, int) else word(v) for v in (threshold, floor)]
    (line,) = ask([f"check {words[0]} {words[1]} {min_samples} {size}"])
    status, _, message = line.partition(" ")
    return int(status), None if message == "-" else message


def key(fingerprint=11, spp=128, bounces=5, matrix=tuple(range(1, 17)), width=37, height=23, seed=7, flags=0, threshold=0.03, floor=0.01, min_samples=32, pass_samples=16):
    """An adaptive key as the dump program reads it."""
    return (fingerprint, spp, bounces, *matrix, width, height, seed, flags, word(threshold), word(floor), min_samples, pass_samples)


def next_pass(started, samples_done, active_pixels, state_key, wanted_key):
    """-> (restart, first_sample, n_samples, whole_pass)"""
    (line,) = ask(["next " + " ".join(str(v) for v in (int(started), samples_done, active_pixels, *state_key, *wanted_key))])
    restart, first, n, whole = (int(v) for v in line.split())
    return bool(restart), first, n, bool(whole)


def complete(cap, samples_done, active_pixels):
    return bool(int(ask([f"complete {cap} {samples_done} {active_pixels}"])[0]))


def refused_flag(flags):
    (line,) = ask([f"flag {flags}"])
    return None if line == "-" else line


def plans(requests):
    """requests: (n_spheres, n_planes, planes_tame, width, local_rows, samples_per_pixel, camera, flags, pass_first_sample, pass_samples)
    -> one dict of the adaptive pass's launch_plan fields each."""
    return [{k: int(v) for k, v in (field.split("=") for field in line.split())} for line in ask(["plan " + " ".join(str(v) for v in r) for r in requests])]
