"""The C ABI of progressive frames (include/rt_hip.h: rt_hip_progress, rt_hip_render_pass_device, rt_hip_render_progressive) where no
device is needed: the POD's layout as a C compiler sees it, and bad arguments refused before anything touches a GPU."""
import ctypes as C
import shutil
import subprocess

import pytest

from rt_amd import capi
from tests.conftest import ROOT


def test_progress_layout_matches_the_header_as_a_c_compiler_sees_it(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "rt_hip.h"', "int main(void) {", 'printf("rt_hip_progress %zu\\n", sizeof(rt_hip_progress));']
    for field, _ in capi.RtHipProgress._fields_:
        lines.append(f'printf("{field} %zu\\n", offsetof(rt_hip_progress, {field}));')
    lines.append("return 0; }")
    source = tmp_path / "layout.c"
    source.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(source), "-o", str(exe)], check=True)
    seen = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(seen["rt_hip_progress"]) == C.sizeof(capi.RtHipProgress) == 16
    assert [name for name, _ in capi.RtHipProgress._fields_] == ["samples_done", "samples_total", "passes", "restarted"]
    for field, _ in capi.RtHipProgress._fields_:
        assert int(seen[field]) == getattr(capi.RtHipProgress, field).offset, field


def test_the_abi_version_stays_and_the_additions_are_exported():
    lib = capi.hip_lib()
    assert lib.rt_hip_abi_version() == 6
    plain = C.CDLL(str(capi.hip_library_path()))  # (as a caller finds them: by name)
    assert hasattr(plain, "rt_hip_render_pass_device") and hasattr(plain, "rt_hip_render_progressive")


def test_bad_arguments_are_refused_without_a_device():
    lib = capi.hip_lib()
    accum, rgba = (C.c_float * 3)(), (C.c_uint32 * 1)()
    # a NULL context, with everything else in order
    assert lib.rt_hip_render_pass_device(None, 1, 1, 0, 0, None, 0, 16, accum, rgba, None, None) == 1
    assert b"NULL" in lib.rt_hip_last_error()
    assert lib.rt_hip_render_progressive(None, None, None, 4, 4, 0, 0, 16, None, None, None) == 1
    assert b"NULL" in lib.rt_hip_last_error()
    # a pass that does not start on a chunk: said before the context is looked at
    for first_sample in (1, 8, 15, 17, 100):
        assert lib.rt_hip_render_pass_device(None, 1, 1, 0, 0, None, first_sample, 16, accum, rgba, None, None) == 1
        message = lib.rt_hip_last_error()
        assert b"multiple of 16" in message and str(first_sample).encode() in message, message
