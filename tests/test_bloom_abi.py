"""Bloom's additions to the C ABI without a GPU: the version stays 6, the five symbols are exported, bound and
described, the PODs are laid out as a C compiler lays them out, no flag bit was added, and what the two device calls refuse BEFORE a
device is touched — NULL arguments, both outputs NULL, sides 0 and above 32768, overlapping buffers, the drop-in's flags — is refused
with the argument's or the flag's name."""
import ctypes as C
import shutil
import subprocess

import pytest

from rt_amd import capi
from tests import bloom_reference as ref
from tests import tonemap_reference as tonemap_ref
from tests.conftest import ROOT

SYMBOLS = ("rt_hip_bloom_default_params", "rt_hip_bloom_from_spec", "rt_hip_bloom_plan", "rt_hip_bloom_device", "rt_hip_render_bloomed")
INVALID_ARGUMENT, UNSUPPORTED = 1, 5
NAN = float("nan")


def last_error() -> str:
    return capi.hip_lib().rt_hip_last_error().decode()


def fake_context():
    """Bytes that are never read as a context: every refusal below comes before the context is looked at.  (A pointer that is not NULL.)"""
    return C.cast(C.create_string_buffer(64), C.c_void_p)


def test_the_version_is_still_6_and_the_symbols_are_exported_bound_and_described():
    lib = capi.hip_lib()
    assert lib.rt_hip_abi_version() == 6 == capi.RT_HIP_ABI_VERSION
    header, integration = (ROOT / "include" / "rt_hip.h").read_text(), (ROOT / "INTEGRATION.md").read_text()
    assert "#define RT_HIP_ABI_VERSION 6" in header
    exported = subprocess.run(["nm", "-D", "--defined-only", str(capi.hip_library_path())], check=True, capture_output=True, text=True).stdout
    bound = {name for name, _, _ in capi.RT_HIP_SYMBOLS}
    for name in SYMBOLS:
        assert f" T {name}\n" in exported, name
        assert name in bound and hasattr(lib, name), name
        assert f"RT_HIP_API rt_hip_status {name}(" in header, name
        assert name in integration, name
    for pod in ("rt_hip_bloom_params", "rt_hip_bloom_info"):
        assert pod in integration


def test_the_pods_are_laid_out_as_a_c_compiler_lays_them_out(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    pods = {"rt_hip_bloom_params": capi.RtHipBloomParams, "rt_hip_bloom_info": capi.RtHipBloomInfo}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "rt_hip.h"', "int main(void) {"]
    for c_name, mirror in pods.items():
        lines.append(f'printf("{c_name} %zu\\n", sizeof({c_name}));')
        for field, _ in mirror._fields_:
            lines.append(f'printf("{c_name}.{field} %zu\\n", offsetof({c_name}, {field}));')
    lines.append("return 0; }")
    source, exe = tmp_path / "layout.c", tmp_path / "layout"
    source.write_text("\n".join(lines))
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(source), "-o", str(exe)], check=True)
    seen = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for c_name, mirror in pods.items():
        assert int(seen[c_name]) == C.sizeof(mirror), c_name
        for field, _ in mirror._fields_:
            assert int(seen[f"{c_name}.{field}"]) == getattr(mirror, field).offset, f"{c_name}.{field}"
    assert C.sizeof(capi.RtHipBloomParams) == 20 and C.sizeof(capi.RtHipBloomInfo) == 24


def test_null_arguments_are_refused():
    lib = capi.hip_lib()
    assert lib.rt_hip_bloom_default_params(None) == INVALID_ARGUMENT and "NULL" in last_error()
    p = capi.RtHipBloomParams()
    assert lib.rt_hip_bloom_from_spec(None, C.byref(p)) == INVALID_ARGUMENT and "NULL" in last_error()
    assert lib.rt_hip_bloom_from_spec(b"default", None) == INVALID_ARGUMENT and "NULL" in last_error()
    assert lib.rt_hip_bloom_plan(4, 4, None, None) == INVALID_ARGUMENT and "rt_hip_bloom_plan: NULL" in last_error()
    assert lib.rt_hip_bloom_device(None, 4, 4, None, None, None, None, None) == INVALID_ARGUMENT and "rt_hip_bloom_device: NULL" in last_error()
    assert lib.rt_hip_bloom_device(fake_context(), 4, 4, None, None, 4096, None, None) == INVALID_ARGUMENT and "rt_hip_bloom_device: NULL" in last_error()
    assert lib.rt_hip_render_bloomed(None, None, None, 4, 4, 1, 0, None, None, None, None, None) == INVALID_ARGUMENT and "rt_hip_render_bloomed: NULL" in last_error()


def test_both_outputs_null_sides_and_overlaps_are_refused_before_the_context_is_looked_at():
    lib, ctx = capi.hip_lib(), fake_context()
    base, frame = 1 << 20, 64 * 36 * 12  # (addresses that are never dereferenced)
    assert lib.rt_hip_bloom_device(ctx, 64, 36, base, None, None, None, None) == INVALID_ARGUMENT
    assert "d_rgb_out and d_layer_out are both NULL" in last_error()
    for width, height in ((0, 36), (64, 0), (32769, 36), (64, 32769), (0xFFFFFFFF, 1)):
        assert lib.rt_hip_bloom_device(ctx, width, height, base, None, base + (1 << 30), None, None) == INVALID_ARGUMENT
        assert last_error() == f"rt_hip_bloom_device: frame {width}x{height} (1 .. 32768 a side)"
    overlaps = [
        ((base, base + 16, None), "d_rgb_out overlaps d_rgb_in"),
        ((base + 16, base, None), "d_rgb_out overlaps d_rgb_in"),
        ((base, base + frame - 4, None), "d_rgb_out overlaps d_rgb_in"),  # the last float
        ((base, None, base), "d_layer_out overlaps d_rgb_in"),
        ((base, base, base + 64), "d_layer_out overlaps d_rgb_in"),
        ((base, base + frame, base + frame + 12), "d_rgb_out"),  # the two outputs on one another
    ]
    for (d_in, d_out, d_layer), words in overlaps:
        assert lib.rt_hip_bloom_device(ctx, 64, 36, d_in, None, d_out, d_layer, None) == INVALID_ARGUMENT
        assert words in last_error() and last_error().startswith("rt_hip_bloom_device: "), (words, last_error())
    assert "only d_rgb_out == d_rgb_in exactly is in place" in last_error() or "d_layer_out" in last_error()
    assert lib.rt_hip_bloom_device(ctx, 64, 36, base + 2, None, base + frame, None, None) == INVALID_ARGUMENT and "not 4-byte aligned" in last_error()


@pytest.mark.parametrize("field,value", [("threshold", NAN), ("threshold", -1.0), ("knee", 2.0), ("knee", NAN), ("intensity", 2000.0), ("intensity", NAN), ("scatter", 1.5), ("scatter", NAN), ("levels", 0), ("levels", 9)])
def test_an_out_of_range_field_is_refused_by_name_before_the_context_is_looked_at(field, value):
    lib = capi.hip_lib()
    p = ref.params(**{field: value})
    status, message = ref.check(p)
    assert status == INVALID_ARGUMENT and f"rt_hip_bloom_params: {field} = " in message
    assert lib.rt_hip_bloom_device(None, 4, 4, None, C.byref(p), None, None, None) == INVALID_ARGUMENT
    assert last_error() == f"rt_hip_bloom_device: {message}"
    assert lib.rt_hip_render_bloomed(None, None, None, 4, 4, 1, 0, C.byref(p), None, None, None, None) == INVALID_ARGUMENT
    assert last_error() == f"rt_hip_render_bloomed: {message}"
    assert lib.rt_hip_bloom_plan(4, 4, C.byref(p), C.byref(capi.RtHipBloomInfo())) == INVALID_ARGUMENT
    assert last_error() == f"rt_hip_bloom_plan: {message}"


def test_the_drop_in_refuses_tone_mapping_s_parameters_by_name_too():
    lib = capi.hip_lib()
    bad = tonemap_ref.params(white=0.0)
    assert lib.rt_hip_render_bloomed(None, None, None, 4, 4, 1, 0, None, C.byref(bad), None, None, None) == INVALID_ARGUMENT
    assert last_error().startswith("rt_hip_render_bloomed: rt_hip_tonemap_params: white = ")
    assert lib.rt_hip_render_bloomed(fake_context(), None, None, 0, 4, 1, 0, None, None, None, None, None) == INVALID_ARGUMENT  # (NULL comes first)
    assert "rt_hip_render_bloomed: NULL" in last_error()


def test_the_drop_in_refuses_flags_by_name_before_the_context_is_looked_at():
    lib, ctx = capi.hip_lib(), fake_context()
    scene, pixels = C.cast(C.create_string_buffer(64), C.c_void_p), 1 << 20  # (neither is read before the flags are)
    refused = [(capi.RT_HIP_FLAG_PREVIEW, "RT_HIP_FLAG_PREVIEW is not available for bloomed frames"), (capi.RT_HIP_FLAG_PERSISTENT_FRAME, "RT_HIP_FLAG_PERSISTENT_FRAME is not available for bloomed frames")]
    refused += [(1 << bit, "unknown flag bits") for bit in (12, 15, 20, 31)]
    for flags, words in refused:
        assert lib.rt_hip_render_bloomed(ctx, C.cast(scene, C.POINTER(capi.RtHipScene)), pixels, 64, 36, 1, flags, None, None, None, None, None) == UNSUPPORTED, hex(flags)
        assert last_error().startswith("rt_hip_render_bloomed: ") and words in last_error(), (hex(flags), last_error())
    for width, height in ((0, 36), (64, 32769)):
        assert lib.rt_hip_render_bloomed(ctx, C.cast(scene, C.POINTER(capi.RtHipScene)), pixels, width, height, 1, 0, None, None, None, None, None) == INVALID_ARGUMENT
        assert last_error() == f"rt_hip_render_bloomed: frame {width}x{height} (1 .. 32768 a side)"


def test_no_flag_bit_was_added():
    header = (ROOT / "include" / "rt_hip.h").read_text()
    assert "BLOOM" not in "".join(line for line in header.splitlines() if "RT_HIP_FLAG_" in line and "#define" in line)
    flags = {name: getattr(capi, name) for name in dir(capi) if name.startswith("RT_HIP_FLAG_")}
    taken = 0
    for value in flags.values():
        taken |= value
    for bit in (12, 15, 20, 31):
        assert not taken & (1 << bit), bit
