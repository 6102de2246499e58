"""Every build of RT_HIP_FLAG_FAST's kernel family that a small frame can reach, held PER PIXEL to the float64 reference.

tests/test_gpu_fast.py holds four full-size frames to whole-frame statistics (within_2e-5 >= 0.99 ...): a FAST build with a handful of
wrong pixels passes it, and so does one that is wrong only at 17 chunks, only in the eye-camera form, or only at 5 spheres + 2 planes —
about a hundred of the fast instantiations were never launched by any test.  Here every case of tests/fast_cases.py is rendered with
RT_HIP_FLAG_FAST plus the case's flags and checked in EVERY pixel against tests/fast_reference.py's rule: |fast - base| <= allowance,
where the allowance is 2e-5 * scale for a pixel none of whose samples can fall the other way at float32 precision and is widened, by
what an ensemble of perturbed float64 runs has seen such a sample change, for a pixel that has one.  tests/test_fast_reference.py shows
on the CPU that the oracle and stand-ins for FAST pass the rule and that wrong tracers do not; tests/test_gpu_fast_math.py ties the
stand-ins' amplitude to the device.

Per frame: stats["kernel"] is the planned kernel (the plan itself is asserted on the CPU and again here); the mean is finite and >= 0 and
alpha is 255; every pixel is within its allowance; tight pixels' packed channels are within 1 of pack(sqrt(base)); the segment count is
within spp x max_bounces x (non-tight pixels) of the oracle's — a DERIVED bound: a tight pixel has no sample that flips, so its paths are
the oracle's, and a non-tight pixel's paths differ by at most all of their segments.  The same call twice gives identical bits.  (That the
multi-GPU group's FAST frame equals the single context's stays asserted in tests/test_gpu_fast.py.)

The last test prints, per sweep, the worst diff / allowance and the number of non-tight pixels (profiles/r26 keeps a copy)."""
import numpy as np
import pytest

import rt_amd
from rt_amd import capi
from tests import fast_cases as cases
from tests import fast_reference as ref

pytestmark = pytest.mark.gpu

FAST = capi.RT_HIP_FLAG_FAST
MEASURED = {}  # sweep: [(case, variant, destination, worst diff / allowance, non-tight pixels)]


def check_frame(case, variant, destination, rgba, rgb, stats, rows=None, segments=True):
    """`rows`: the frame rows this frame holds (a stripe partition), all of them otherwise."""
    rule = cases.reference(case.name)
    take = slice(None) if rows is None else rows
    base, allowance, tight = rule.base[take], rule.allowance[take], rule.tight[take]
    what = f"{case.name}, {variant.label}, {destination}"
    assert stats["kernel"] == variant.kernel, (what, stats["kernel"])
    assert np.isfinite(rgb).all() and (rgb >= 0).all() and np.all((rgba & 0xFF) == 0xFF), what
    excess = np.abs(rgb.astype(np.float64) - base).max(axis=-1) / allowance
    MEASURED.setdefault(case.sweep, []).append((case.name, variant.label, destination, float(excess.max()), int((~tight).sum())))
    beyond = np.argwhere(excess > 1.0)
    assert beyond.size == 0, f"{what}: {len(beyond)} of {excess.size} pixels beyond their allowance; the first at (y, x) = {tuple(beyond[0])}: diff / allowance = {excess[tuple(beyond[0])]:.3f} (tight: {bool(tight[tuple(beyond[0])])})"
    levels = np.abs(ref.channels(rgba) - ref.pack(base)).max(axis=-1)
    assert (levels[tight] <= 1).all(), f"{what}: {int((levels[tight] > 1).sum())} tight pixels whose packed channels are more than 1 from pack(sqrt(base))"
    if segments:
        assert abs(stats["segments"] - cases.oracle_frame(case.name)[2]) <= case.spp * case.bounces * int((~rule.tight).sum()), (what, stats["segments"], cases.oracle_frame(case.name)[2])


def into_page_locked_memory(tracer, case, variant):
    """rt_hip_render, twice: the frame, and that the second call's is the same bits"""
    pod = cases.pod_of(case)
    cases.assert_plan(case, variant, 1)
    rgba, rgb, stats = tracer.render(pod, case.width, case.height, seed=case.seed, flags=FAST | variant.flags, want_rgb=True)
    check_frame(case, variant, "page-locked", rgba, rgb, stats)
    again_rgba, again_rgb, again = tracer.render(pod, case.width, case.height, seed=case.seed, flags=FAST | variant.flags, want_rgb=True)
    assert np.array_equal(rgba, again_rgba) and np.array_equal(rgb.view(np.uint32), again_rgb.view(np.uint32)) and stats["segments"] == again["segments"], f"{case.name}, {variant.label}: the same call twice"


def render_device(tracer, case, variant, partition=None):
    """rt_hip_render_device into tensors: (rgba8, float mean, stats) of the rows the call owns"""
    import torch

    rows = case.height if partition is None else rt_amd.local_rows(case.height, *partition)
    padded = case.height if partition is None else rt_amd.padded_local_rows(case.height, partition[1], partition[2])
    frame = torch.full((padded, case.width), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    mean = torch.full((padded, case.width, 3), float("nan"), dtype=torch.float32, device="cuda:0")
    tracer.render_device(case.width, case.height, frame.data_ptr(), seed=case.seed, flags=FAST | variant.flags, partition=partition, d_rgb_f32=mean.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return frame.cpu().numpy().view(np.uint32)[:rows], mean.cpu().numpy()[:rows], tracer.stats()


def into_hbm(tracer, case, variant):
    cases.assert_plan(case, variant, 0)
    tracer.upload(cases.pod_of(case))
    rgba, rgb, stats = render_device(tracer, case, variant)
    check_frame(case, variant, "HBM", rgba, rgb, stats)


def in_stripes(tracer, case, variant):
    """partition = (rank, 3, 5): each rank's rows held to the same rows of the whole frame's allowance; the segments add up to a frame's"""
    tracer.upload(cases.pod_of(case))
    total = 0
    for rank in range(3):
        rows = cases.stripe_rows(case.height, rank)
        cases.assert_plan(case, variant, 0, len(rows))
        rgba, rgb, stats = render_device(tracer, case, variant, partition=(rank, 3, 5))
        assert rgba.shape[0] == len(rows)
        check_frame(case, variant, f"stripes of rank {rank}", rgba, rgb, stats, rows=rows, segments=False)
        total += stats["segments"]
    rule = cases.reference(case.name)
    assert abs(total - cases.oracle_frame(case.name)[2]) <= case.spp * case.bounces * int((~rule.tight).sum()), (case.name, variant.label, total)


def check_case(tracer, case):
    for variant in case.variants:
        into_page_locked_memory(tracer, case, variant)
        if case.hbm:
            into_hbm(tracer, case, variant)
        if case.stripes:
            in_stripes(tracer, case, variant)


@pytest.mark.parametrize("name", [case.name for case in cases.of_sweep("builds")])
def test_every_scalar_register_build_in_both_camera_forms_and_both_item_forms(tracer, name):
    """26 (spheres, planes) pairs x {pinhole, eye} x {whole chunks, HALF} at 37 x 23; six pairs also into HBM tiles, three in stripes."""
    check_case(tracer, cases.BY_NAME[name])


@pytest.mark.parametrize("name", [case.name for case in cases.of_sweep("chunks")])
def test_the_chunk_counts_from_2_to_33(tracer, name):
    """13 x 7, 17 ... 520 samples: one scalar-register build and the forced resident kernel, whole and auto (HALF up to K = 16), across the
    tile sizes and both ways a tile is folded."""
    check_case(tracer, cases.BY_NAME[name])


@pytest.mark.parametrize("name", [case.name for case in cases.of_sweep("kernels")])
def test_the_resident_forms_and_the_rolling_kernels(tracer, name):
    """FORCE_RESIDENT (pinhole; orthographic = the general camera; the scalar-load scan with a plane), FORCE_TILED and FORCE_STREAMED, each
    in whole chunks, forced HALF and auto."""
    check_case(tracer, cases.BY_NAME[name])


def test_what_was_measured(capsys):
    """Per sweep: the frames rendered, the worst diff / allowance among them and where, the non-tight pixels of the frame it was in."""
    with capsys.disabled():
        print("\nsweep: frames | worst diff / allowance (case, variant, destination) | non-tight pixels: fewest .. most per frame")
        for sweep, rows in MEASURED.items():
            worst = max(rows, key=lambda row: row[3])
            print(f"  {sweep}: {len(rows)} | {worst[3]:.3f} ({worst[0]}, {worst[1]}, {worst[2]}) | {min(r[4] for r in rows)} .. {max(r[4] for r in rows)}")
    assert all(row[3] <= 1.0 for rows in MEASURED.values() for row in rows)
