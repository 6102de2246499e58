"""The scatter tail's rare branches on the GPU: every constructed case of tests/rare_cases.py — the re-draw of a zero random vector, lambert's
approx_zero rule on both sides of its threshold and of the wave vote in front of it, the zero pixel jitter, a sphere and a plane at equal
distance, material values that send NaN, negative and infinite means to the pack — through every family of the render kernel an 8 x 8 frame
can be steered to, against oracle.render: packed pixels and float mean as uint32, segments, tolerance 0.  These branches are compiled into
every instantiation of render_queue separately, and the frames of the rest of the suite do not reach them (profiles/r18/branch_census.txt).

That a case DOES reach its branch, and that its target pixel depends on it, is asserted on the CPU from the oracle's census
(tests/test_rare_branches.py); nothing here is judged by what the kernels return.  RT_HIP_FLAG_FAST is not bit-exact by contract and stays out."""
import numpy as np
import pytest

from rt_amd import capi
from tests import adaptive_reference as adaptive_ref
from tests import rare_cases as rc
from tests import test_gpu_adaptive as adaptive_tests
from tests import test_gpu_progressive as progressive_tests

pytestmark = pytest.mark.gpu

W, H = rc.W, rc.H
SM = capi.RT_HIP_FLAG_SM_MATERIALS
RESIDENT, TILED, STREAMED = capi.RT_HIP_FLAG_FORCE_RESIDENT, capi.RT_HIP_FLAG_FORCE_TILED, capi.RT_HIP_FLAG_FORCE_STREAMED
HALF, WHOLE = capi.RT_HIP_FLAG_FORCE_HALF_CHUNKS, capi.RT_HIP_FLAG_FORCE_WHOLE_CHUNKS
BVH = capi.RT_HIP_FLAG_BVH
BOXES = capi.RT_HIP_FLAG_TRACE_BOXES
BOX_TREE = BOXES | capi.RT_HIP_FLAG_BOX_BVH
ONE_SHOT = {"auto": 0, "resident": RESIDENT, "tiled": TILED, "streamed": STREAMED, "half": HALF, "whole": WHOLE, "half_resident": HALF | RESIDENT, "bvh": BVH, "boxes": BOXES, "box_tree": BOX_TREE}


def expected_kernel(pod, flags, passes=False):
    """The kernel rt_amd/csrc/launch_plan.cpp (choose_kernel, plan_launch) names for an 8 x 8 frame of `pod`: every case's camera has an eye
    and its planes are of ordinary size."""
    primitives = pod.n_spheres + pod.n_planes
    if flags & BVH:
        kernel = "bvh"
    elif flags & STREAMED:
        kernel = "streamed"
    elif flags & TILED:
        kernel = "tiled"
    elif not (flags & RESIDENT) and pod.n_spheres >= 1 and pod.n_planes <= 3 and primitives <= 8:
        kernel = "small"
    else:
        kernel = "resident"
    if passes or ((flags & BOXES) and pod.n_boxes):  # the pass and box builds are builds of the two tile-per-wave kernels
        kernel = "bvh" if kernel in ("bvh", "streamed") else "resident"
    if (flags & BOX_TREE) == BOX_TREE and pod.n_boxes:
        kernel = "bvh"
    return kernel


def assert_same(case, what, rgba, rgb, want_rgba, want_rgb):
    if not rc.same_bits(rgb, want_rgb, nan_ok=case.nan_ok):
        bad = np.argwhere((rgb.view(np.uint32) != want_rgb.view(np.uint32)).any(axis=-1))
        y, x = bad[0]
        raise AssertionError(f"{case.name}, {what}: float mean differs in {len(bad)} of {W * H} pixels; first at (x={x}, y={y}): gpu {rgb[y, x]} vs oracle {want_rgb[y, x]}"
                             + (f" (the case's event is in pixel {case.target_xy})" if case.target is not None else ""))
    assert np.array_equal(rgba, want_rgba), f"{case.name}, {what}: {(rgba != want_rgba).sum()} packed pixels differ"


@pytest.mark.parametrize("name,sm", rc.CASE_TABLES)
def test_one_shot_through_every_family(tracer, name, sm):
    """auto, the three forced kernels, half and whole chunks, the sphere hierarchy (cases with spheres), one box off to the side linearly and
    through the box hierarchy — each under the case's scatter table, each naming the kernel the launch plan says."""
    case = rc.case(name)
    want_rgba, want_rgb, want_segments = rc.reference(name, sm)
    table = SM if sm else 0
    ran = set()
    for family, flags in ONE_SHOT.items():
        if family == "bvh" and not case.spheres:
            continue
        pod = case.pod(boxes=bool(flags & BOXES))
        rgba, rgb, stats = tracer.render(pod, W, H, seed=case.seed, flags=flags | table, want_rgb=True)
        assert stats["kernel"] == expected_kernel(pod, flags), (name, family, stats["kernel"])
        assert_same(case, f"{family} ({stats['kernel']})", rgba, rgb, want_rgba, want_rgb)
        assert stats["segments"] == want_segments and stats["primary_samples"] == W * H * case.spp, (name, family, stats)
        ran.add(stats["kernel"])
    assert ran >= ({"resident", "tiled", "streamed", "bvh"} | ({"small"} if case.spheres else set())), (name, ran)


def pass_size_of(case):
    """Passes are whole chunks of 16 samples: the largest size whose first boundary lies at or before the event's sample — the event is
    then in the SECOND pass (cases whose event is in the first 16 samples have one pass, or the event in the first)."""
    return max(16, 16 * (case.sample // 16))


def test_the_pass_boundaries_put_late_events_into_the_second_pass():
    late = [c for c in rc.all_cases() if c.target is not None and c.sample >= 16]
    assert {"redraw_lambert", "redraw_metal", "redraw_lambert_sample40", "redraw_second_scatter_wall", "redraw_second_scatter_wall_metal", "approx_zero_sample17"} <= {c.name for c in late}
    assert any(c.name.startswith("zero_jitter") for c in late)
    for c in late:
        size = pass_size_of(c)
        assert size <= c.sample < min(2 * size, c.spp) and c.spp > size, (c.name, size, c.sample, c.spp)


@pytest.mark.parametrize("name,sm", rc.CASE_TABLES)
def test_progressive_passes(tracer, name, sm):
    """rt_hip_render_progressive: after every pass the frame is the oracle's at samples_done; an event at sample 16 or later happens in the
    second pass (the pass builds start a pixel's streams at first_chunk, not at 0)."""
    case = rc.case(name)
    table = SM if sm else 0
    pod, size = case.pod(), pass_size_of(case)
    progressive_tests.abandon_the_frame_in_flight(tracer)
    done, segments = 0, 0
    while done < case.spp:
        rgba, rgb, stats, progress = tracer.render_progressive(pod, W, H, seed=case.seed, flags=table, pass_samples=size, want_rgb=True)
        this = min(size, case.spp - done)
        done += this
        assert progress["samples_done"] == done and progress["samples_total"] == case.spp, (name, progress)
        assert stats["kernel"] == expected_kernel(pod, 0, passes=True) and stats["primary_samples"] == W * H * this, (name, stats)
        want_rgba, want_rgb, _ = rc.reference(name, sm, done)
        assert_same(case, f"progressive, {done} of {case.spp} samples", rgba, rgb, want_rgba, want_rgb)
        segments += stats["segments"]
    assert segments == rc.reference(name, sm)[2]


@pytest.mark.parametrize("name,sm", rc.CASE_TABLES)
def test_adaptive_passes_that_stop_nobody(tracer, name, sm):
    """rt_hip_render_adaptive with min_samples above the cap: the adaptive builds trace every pixel in every pass, and after every pass
    the frame is the oracle's at samples_done."""
    case = rc.case(name)
    table = SM if sm else 0
    pod, size = case.pod(), pass_size_of(case)
    params = adaptive_ref.params(min_samples=4096)
    adaptive_tests.abandon_the_accumulation_in_flight(tracer)
    done, segments = 0, 0
    while done < case.spp:
        rgba, rgb, counts, stats, info = tracer.render_adaptive(pod, W, H, seed=case.seed, flags=table, pass_samples=size, params=params, want_rgb=True)
        done += min(size, case.spp - done)
        assert info["samples_done"] == done and (counts == done).all() and info["complete"] == int(done == case.spp), (name, info)
        assert stats["kernel"] == expected_kernel(pod, 0, passes=True), (name, stats)
        want_rgba, want_rgb, _ = rc.reference(name, sm, done)
        assert_same(case, f"adaptive, {done} of {case.spp} samples", rgba, rgb, want_rgba, want_rgb)
        segments += stats["segments"]
    assert segments == rc.reference(name, sm)[2]
