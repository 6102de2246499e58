"""The sixteen light builds of render_queue — eight under RT_HIP_FLAG_EMISSION, eight under RT_HIP_FLAG_DIRECT_LIGHT
(§3.13) — across the chunk count K = ceil(samples / 16), on ragged frames.  Modelled on tests/test_gpu_chunk_sweep.py, which holds every
OTHER build family over this axis: how a tile is cut, which way fold_tile folds it and how large the chunk-sum slots are change with K
behind tables that differ from build to build, and in the direct builds end_sample adds `direct` in front of that fold.

Frames are 13 x 7: ragged against every tile shape (16 x 4 ... 4 x 1 page-locked, 8 x 8 ... 2 x 2 in HBM), with waves that have no tile.
Every build — the LDS scan through a pinhole and a tilted camera, the scalar-load scan, the hierarchy, each under the mg and the sm table
— renders 16, 17, 48, 80, 256, 272, 520 and 4096 samples (K = 1, 2, 3, 5, 16, 17, 33, 256: the K at which pixels_log2 steps 6, 5, 4, 3,
2, a wave first owns more than 128 items, and the slots are largest), through rt_hip_render (a page-locked frame) and through
rt_hip_render_device (tensors in HBM).  Tolerance 0 — packed pixels and float mean as uint32, segments, primary_samples, kernel_variant —
against tests.light_reference.render / tests.direct_reference.render, never against another GPU frame.  Before each frame the CPU plan
dump (tests/light_plan.py) is asked for build, K, pixels_log2, tile and fold path, and the test asserts them; the last test prints the
cells each build took.

The direct frames exercise the protocol: per scene the census of tests/direct_reference.py says that vertices aimed and aimed at nothing,
that shadow queries came back visible and occluded, and that a sampled light was met behind a vertex that had sampled it."""
import functools

import numpy as np
import pytest

import rt_amd
from oracle import binding as oracle
from tests import direct_reference as direct_ref
from tests import light_plan
from tests import light_reference as light_ref
from tests.test_gpu_chunk_sweep import refused_and_nothing_launched, render_into_hbm, same_frame

pytestmark = pytest.mark.gpu

W, H = 13, 7
SEED = 23
UNSUPPORTED = 5
EMISSION, DIRECT, SM, BVH = light_plan.EMISSION, light_plan.DIRECT, light_plan.SM, light_plan.BVH
FLAGS = {"lights": EMISSION, "direct": DIRECT}
# spp: (K, pixels_log2 in whole chunks — the light builds have no HALF build)
SAMPLES = {16: (1, 6), 17: (2, 5), 48: (3, 4), 80: (5, 3), 256: (16, 2), 272: (17, 2), 520: (33, 2), 4096: (256, 2)}
LAMBERT, METAL, DIELECTRIC = light_ref.LAMBERT, light_ref.METAL, light_ref.DIELECTRIC
MATERIALS = [(LAMBERT, (0.8, 0.8, 0.3), 0.0, 1.0), (METAL, (0.9, 0.6, 0.4), 0.2, 0.9), (DIELECTRIC, (0.9, 0.95, 1.0), 0.0, 1.5), (LAMBERT, (0.3, 0.5, 0.8), 0.0, 0.8), (LAMBERT, (0.5, 0.5, 0.5), 0.0, 1.0)]
LAMP = 4
TABLE = np.array([(0, 0, 0)] * 4 + [(4, 3.2, 2)], dtype=np.float32)
PLANE = [(0, 1, 0, 0, 0)]
# a lamp, a lambert sphere, a metal sphere and a dielectric one (glass under the sm table) over a plane
SMALL = [(1.6, 2.6, -0.4, 0.6, LAMP), (-0.9, 0.7, -0.2, 0.7, 3), (0.9, 0.45, 0.6, 0.45, 1), (-0.1, 0.4, 1.6, 0.4, 2)]
CAMERAS = {"pinhole": ((0.3, 1.5, 5.0), (0, 0, -1)), "tilted": ((0.3, 1.5, 5.0), (0.2, -0.15, -1))}


@functools.lru_cache(maxsize=None)
def camera(name):
    return rt_amd.Scene.parse("").set_camera(*CAMERAS[name]).describe(W, H)


def small(spp, bounces=6, view="pinhole"):
    return light_ref.scene_pod(camera(view), spheres=SMALL, planes=PLANE, spp=spp, bounces=bounces, materials=MATERIALS)


def field48(spp, bounces=6):
    """the small scene plus 44 little spheres on the ground behind it: 48 spheres, the scalar-load scan (it starts at 40)"""
    spheres = SMALL + [((i % 11 - 5) * 0.45, 0.15, -1.5 - (i // 11) * 0.5, 0.15, i % 4) for i in range(44)]
    return light_ref.scene_pod(camera("pinhole"), spheres=spheres, planes=PLANE, spp=spp, bounces=bounces, materials=MATERIALS)


def field300(spp, bounces=6):
    """300 spheres of which every sixtieth — 5 — is a lamp, larger and lifted above the field, for the hierarchy"""
    spheres = [(x, 1.2, z + 2.0, 0.3, LAMP) if i % 60 == 7 else (x, y, z + 2.0, r, i % 4) for i, (x, y, z, r, _) in enumerate(light_ref.grid_spheres(300, radius=0.1, pitch=0.25))]
    return light_ref.scene_pod(camera("pinhole"), spheres=spheres, planes=PLANE, spp=spp, bounces=bounces, materials=MATERIALS)


# scan: (scene, flags beside the light flags, the camera form the LDS scan is compiled for | None)
SCANS = {
    "LDS scan, pinhole": (lambda spp, bounces=6: small(spp, bounces, "pinhole"), 0, "pinhole"),
    "LDS scan, general camera": (lambda spp, bounces=6: small(spp, bounces, "tilted"), 0, "eye"),
    "scalar-load scan": (field48, 0, None),
    "hierarchy": (field300, BVH, None),
}


@functools.lru_cache(maxsize=None)
def reference(scan, flag, spp, sm, bounces=6):
    """Computed once per (scene, flag, samples, table), shared by both entry points, read-only."""
    pod = SCANS[scan][0](spp, bounces)
    render = direct_ref.render if flag == "direct" else light_ref.render
    rgba, rgb, stats = render(pod, W, H, TABLE, seed=SEED, sm_materials=sm)
    rgba.setflags(write=False), rgb.setflags(write=False)
    return rgba, rgb, stats["segments"]


def planned(scan, flag, spp, sm, host, bounces=6):
    """The plan of a sweep frame, held to the tables above: the build, K, pixels_log2, the tile's shape and the fold path."""
    make, extra, form = SCANS[scan]
    pod = make(spp, bounces)
    if form is not None:
        assert oracle.primary_ray(pod, W, H, 0, 0, want_form=True)[2] == form
    p = light_plan.planned(pod, TABLE, W, H, FLAGS[flag] | extra | (SM if sm else 0), host)
    chunks, pixels_log2 = SAMPLES[spp]
    assert p["refusal"] == "" and light_plan.build_name(p) == f"{flag} ({scan}, {'sm' if sm else 'mg'})", (scan, flag, spp, sm, p)
    assert (p["chunks"], p["pixels_log2"], p["halves"], p["sub_chunk_items"]) == (chunks, pixels_log2, 0, 0), (scan, flag, spp, p)
    # a page-locked frame is cut into tiles 16 wide at the most (every row fragment is a PCIe write), a frame in HBM into tiles near square
    assert p["tile_w_log2"] == (min(4, pixels_log2) if host else (pixels_log2 + 1) // 2), (scan, flag, spp, host, p)
    tile_w, tile_h = 1 << p["tile_w_log2"], 1 << (pixels_log2 - p["tile_w_log2"])
    assert (p["tiles_x"], p["tiles_y"]) == (-(-W // tile_w), -(-H // tile_h)) and (W % tile_w or H % tile_h), (scan, flag, spp, host, p)  # ragged
    assert p["slot_bytes"] == 4 * (chunks << pixels_log2) * 12 and (light_plan.fold_path(p) == "channel-per-lane") == (pixels_log2 <= 4)
    return p


def cell(p, host):
    return (p["chunks"], p["pixels_log2"], f"{1 << p['tile_w_log2']}x{1 << (p['pixels_log2'] - p['tile_w_log2'])}", light_plan.fold_path(p), "page-locked" if host else "HBM")


def check_frame(tracer, scan, flag, spp, sm, bounces=6):
    make, extra, _ = SCANS[scan]
    pod = make(spp, bounces)
    flags = FLAGS[flag] | extra | (SM if sm else 0)
    want_rgba, want_rgb, want_segments = reference(scan, flag, spp, sm, bounces)
    tracer.set_emission(TABLE)
    for host in (1, 0):
        p = planned(scan, flag, spp, sm, host, bounces)
        rgba, rgb, stats = tracer.render(pod, W, H, seed=SEED, flags=flags, want_rgb=True) if host else render_into_hbm(tracer, pod, W, H, SEED, flags)
        what = f"{light_plan.build_name(p)}, {spp} spp, {'rt_hip_render' if host else 'rt_hip_render_device'}"
        assert stats["kernel"] == light_plan.kernel_of(p) and stats["primary_samples"] == W * H * spp, (what, stats)
        same_frame(rgba, rgb, want_rgba, want_rgb, what)
        assert stats["segments"] == want_segments, (what, stats["segments"], want_segments)


@pytest.fixture(autouse=True)
def _no_table_outlives_a_test(tracer):
    yield
    tracer.set_emission(None)  # (the session's context is shared: no other test file sees a table)


# ---- the sweep ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spp", list(SAMPLES))
@pytest.mark.parametrize("sm", [False, True], ids=["mg", "sm"])
@pytest.mark.parametrize("scan", list(SCANS))
@pytest.mark.parametrize("flag", list(FLAGS))
def test_every_light_build_across_the_chunk_count(tracer, flag, scan, sm, spp):
    check_frame(tracer, scan, flag, spp, sm)


@pytest.mark.parametrize("sm", [False, True], ids=["mg", "sm"])
@pytest.mark.parametrize("scan", list(SCANS))
@pytest.mark.parametrize("flag", list(FLAGS))
def test_long_paths_at_three_chunks(tracer, flag, scan, sm):
    """max_bounces = 50 at K = 3, the first channel-per-lane fold: paths run long, under the direct flag with two steps per lambert vertex."""
    check_frame(tracer, scan, flag, 48, sm, bounces=50)


def test_fifty_bounces_make_longer_paths():
    for scan in SCANS:
        assert reference(scan, "direct", 48, False, 50)[2] > reference(scan, "direct", 48, False)[2], scan


# ---- the direct frames exercise the protocol -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sm", [False, True], ids=["mg", "sm"])
@pytest.mark.parametrize("scan", list(SCANS))
def test_the_direct_frames_exercise_the_protocol(scan, sm):
    """From the restatement's census, per scene, at three chunks: vertices that aimed and that aimed at nothing, shadow queries that came
    back visible and occluded, a sampled light met behind a vertex that had sampled it; and the census frame is the sweep's reference."""
    pod = SCANS[scan][0](48)
    assert direct_ref.count(pod, TABLE) == (5 if scan == "hierarchy" else 1)
    rgba, rgb, stats, _, own, _ = direct_ref.render_census(pod, W, H, TABLE, seed=SEED, sm_materials=sm)
    want_rgba, want_rgb, want_segments = reference(scan, "direct", 48, sm)
    assert rgba.tobytes() == want_rgba.tobytes() and rgb.tobytes() == want_rgb.tobytes() and stats["segments"] == want_segments
    print(f"{scan}, {'sm' if sm else 'mg'}: {own}")
    for event in ("vertex_aimed", "vertex_not_aimed", "shadow_visible", "shadow_occluded", "sampled_light_after_sampling_vertex"):
        assert own[event] > 0, (scan, sm, event, own)
    # (and the flag and the table tell the frames apart: what makes the sm frames a test of the sm builds, the direct frames of the direct builds)
    assert not np.array_equal(want_rgba, reference(scan, "lights", 48, sm)[0]) and not np.array_equal(want_rgba, reference(scan, "direct", 48, not sm)[0])


# ---- the one-shot limit ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scan", ["LDS scan, pinhole", "hierarchy"])
@pytest.mark.parametrize("flag", list(FLAGS))
def test_the_one_shot_limit_of_4096_samples(tracer, flag, scan):
    """4097 samples are refused under the flags as they are without them: the message names the count and the limit, nothing is launched,
    through either entry point, and the context renders on."""
    import torch

    make, extra, _ = SCANS[scan]
    pod = make(4097)
    flags = FLAGS[flag] | extra
    tracer.set_emission(TABLE)
    check_frame(tracer, scan, flag, 16, False)
    before = tracer.stats()
    refused_and_nothing_launched(tracer, pod, W, H, flags, "4097", "4096")
    tracer.upload(pod)
    frame = torch.full((H, W), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    with pytest.raises(rt_amd.RtHipError) as refused:
        tracer.render_device(W, H, frame.data_ptr(), seed=SEED, flags=flags, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert refused.value.status == UNSUPPORTED and "4097" in str(refused.value) and "4096" in str(refused.value) and bool((frame == 0x5A5A5A5A).all())
    now = tracer.stats()
    assert (now["segments"], now["kernel"], now["primary_samples"]) == (before["segments"], before["kernel"], before["primary_samples"])
    check_frame(tracer, scan, flag, 17, False)


# ---- what ran ----------------------------------------------------------------------------------------------------------------------------
def test_every_light_build_is_swept_at_every_chunk_count(capsys):
    """The cases above, asked of the plan dump once more: per build the (K, pixels_log2, tile, fold path, entry point) its frames take —
    all sixteen builds, each at every K of the sweep through both entry points."""
    ran = {}
    for flag in FLAGS:
        for scan in SCANS:
            for sm in (False, True):
                for spp in SAMPLES:
                    for host in (1, 0):
                        p = planned(scan, flag, spp, sm, host)
                        ran.setdefault(light_plan.build_name(p), set()).add(cell(p, host))
    with capsys.disabled():
        print("\nbuild: (K, pixels_log2, tile, fold path, frame) of the frames of tests/test_gpu_light_chunk_sweep.py")
        for build in sorted(ran):
            print(f"  {build}: " + ", ".join(f"({k}, {log2}, {tile}, {fold}, {frame})" for k, log2, tile, fold, frame in sorted(ran[build])))
    assert sorted(ran) == sorted(light_plan.BUILDS["lights"] + light_plan.BUILDS["direct"])
    for build, cells in ran.items():
        assert {(k, log2, frame) for k, log2, _, _, frame in cells} == {(k, log2, frame) for k, log2 in SAMPLES.values() for frame in ("page-locked", "HBM")}, (build, cells)
        assert any(fold == "per-pixel" and k > 1 for k, _, _, fold, _ in cells) and any(fold == "channel-per-lane" and log2 == 2 and k > 32 for k, log2, _, fold, _ in cells)
