"""tests/native/pass_plan_dump.cpp, built once per test process: the host-only policy of progressive frames (the launch plan of a
pass, the sequencing of passes, the flags a pass takes) asked on the CPU.  Shared by tests/test_pass_plan.py, which pins the policy,
and tests/test_gpu_progressive.py, which asks it which tile shape — and so which fold path of the kernel — a pass of its frames takes."""
import functools
import shutil
import subprocess
import tempfile

from tests.conftest import ROOT

SOURCES = [str(ROOT / "tests" / "native" / "pass_plan_dump.cpp"), str(ROOT / "rt_amd" / "csrc" / "launch_plan.cpp"), str(ROOT / "rt_amd" / "csrc" / "progressive.cpp")]


@functools.lru_cache(maxsize=None)
def executable():
    """The dump program, built with g++ alone (nothing of ROCm on the command line); None without a compiler."""
    cxx = shutil.which("g++")
    if cxx is None:
        return None
    exe = tempfile.mkdtemp(prefix="pass_plan_") + "/pass_plan_dump"
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


def plans(requests):
    """requests: (n_spheres, n_planes, planes_tame, width, local_rows, samples_per_pixel, camera, flags, host_frame, fast, pass_first_sample,
    pass_samples) -> one dict of every launch_plan field each."""
    return [{k: int(v) for k, v in (field.split("=") for field in line.split())} for line in ask(["plan " + " ".join(str(v) for v in r) for r in requests])]


def key(fingerprint=11, spp=100, bounces=5, matrix=tuple(range(1, 17)), width=37, height=23, seed=7, flags=0):
    """A frame key as the dump program reads it (the matrix as 16 words)."""
    return (fingerprint, spp, bounces, *matrix, width, height, seed, flags)


def next_pass(started, samples_done, state_key, request_key, pass_samples):
    """-> (restart, first_sample, n_samples, complete)"""
    (line,) = ask(["next " + " ".join(str(v) for v in (int(started), samples_done, *state_key, *request_key, pass_samples))])
    restart, first, n, complete = (int(v) for v in line.split())
    return bool(restart), first, n, bool(complete)


def refused_flag(flags):
    (line,) = ask([f"flag {flags}"])
    return None if line == "-" else line
