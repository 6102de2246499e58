"""The C ABI of the denoiser (include/rt_hip.h: rt_hip_denoise_params, rt_hip_denoise_default_params, rt_hip_guide_device,
rt_hip_denoise_device, rt_hip_denoise_progressive) where no device is needed: the symbols, the POD's layout as a C compiler sees it,
bad arguments and bad parameters refused before anything touches a GPU, and rt_headless' --denoise without --progressive."""
import ctypes as C
import math
import shutil
import subprocess

import pytest

from rt_amd import capi, renderer
from tests.conftest import ROOT

SYMBOLS = ["rt_hip_denoise_default_params", "rt_hip_guide_device", "rt_hip_denoise_device", "rt_hip_denoise_progressive"]
INVALID_ARGUMENT = 1


def test_the_abi_version_stays_and_the_four_additions_are_exported_and_bound():
    lib = capi.hip_lib()
    assert lib.rt_hip_abi_version() == 6
    plain = C.CDLL(str(capi.hip_library_path()))  # (as a caller finds them: by name)
    bound = {name for name, _, _ in capi.RT_HIP_SYMBOLS}
    for name in SYMBOLS:
        assert hasattr(plain, name), f"{name} is not exported"
        assert name in bound, f"{name} is not bound in rt_amd/capi.py"
    integration = (ROOT / "INTEGRATION.md").read_text()
    assert all(name in integration for name in SYMBOLS)


def test_params_layout_matches_the_header_as_a_c_compiler_sees_it(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc is not None, "no C compiler"
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "rt_hip.h"', "int main(void) {", 'printf("rt_hip_denoise_params %zu\\n", sizeof(rt_hip_denoise_params));']
    for field, _ in capi.RtHipDenoiseParams._fields_:
        lines.append(f'printf("{field} %zu\\n", offsetof(rt_hip_denoise_params, {field}));')
    lines.append("return 0; }")
    source = tmp_path / "layout.c"
    source.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(source), "-o", str(exe)], check=True)
    seen = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(seen["rt_hip_denoise_params"]) == C.sizeof(capi.RtHipDenoiseParams) == 20
    assert [name for name, _ in capi.RtHipDenoiseParams._fields_] == ["iterations", "normal_squarings", "sigma_colour", "sigma_albedo", "sigma_depth"]
    for field, _ in capi.RtHipDenoiseParams._fields_:
        assert int(seen[field]) == getattr(capi.RtHipDenoiseParams, field).offset, field


def test_null_arguments_are_refused_without_a_device():
    lib = capi.hip_lib()
    buffer = (C.c_float * 8)()
    assert lib.rt_hip_denoise_default_params(None) == INVALID_ARGUMENT and b"NULL" in lib.rt_hip_last_error()
    assert lib.rt_hip_guide_device(None, 1, 1, 0, buffer, None) == INVALID_ARGUMENT and b"NULL" in lib.rt_hip_last_error()
    assert lib.rt_hip_denoise_device(None, 1, 1, buffer, buffer, None, buffer, None, None) == INVALID_ARGUMENT and b"NULL" in lib.rt_hip_last_error()
    assert lib.rt_hip_denoise_progressive(None, None, buffer, None, None) == INVALID_ARGUMENT and b"NULL" in lib.rt_hip_last_error()


def test_the_defaults_are_in_range():
    p = renderer.denoise_default_params()
    assert 0 <= p.iterations <= 6 and 0 <= p.normal_squarings <= 8
    assert all(math.isfinite(s) and s > 0 for s in (p.sigma_colour, p.sigma_albedo, p.sigma_depth))


BAD = [("iterations", 7), ("iterations", 2**31), ("normal_squarings", 9), ("sigma_colour", 0.0), ("sigma_colour", -1.0), ("sigma_colour", float("nan")), ("sigma_albedo", float("inf")), ("sigma_albedo", -0.0),
       ("sigma_depth", float("nan")), ("sigma_depth", -2.5)]


@pytest.mark.parametrize("field,value", BAD)
def test_every_out_of_range_parameter_is_refused_with_its_fields_name_before_the_context_is_looked_at(field, value):
    lib = capi.hip_lib()
    p = renderer.denoise_default_params()
    setattr(p, field, value)
    buffer = (C.c_float * 8)()
    for call in (lambda: lib.rt_hip_denoise_device(None, 1, 1, buffer, buffer, C.byref(p), buffer, None, None), lambda: lib.rt_hip_denoise_progressive(None, C.byref(p), buffer, None, None)):
        assert call() == INVALID_ARGUMENT
        message = lib.rt_hip_last_error().decode()
        assert field in message and "NULL" not in message, message


def test_headless_denoise_without_progressive_exits_2():
    binary = ROOT / "rt_amd" / "bin" / "rt_headless"
    out = subprocess.run([str(binary), "--scene", "basic.toml", "--denoise"], cwd=ROOT, capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "--denoise" in out.stderr and "--progressive" in out.stderr, (out.returncode, out.stderr)
