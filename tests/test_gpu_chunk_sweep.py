"""The tile-per-wave builds of the render kernel across the chunk count K = ceil(samples / 16), up to the one-shot limit of 4096 samples.

How a tile is cut depends on K: it holds K << pixels_log2 items, pixels_log2 falls from 6 to 2 as K grows, from 4 downwards fold_tile
folds one channel per lane instead of one pixel per lane, up to K = 16 short launches take the HALF build, beyond K = 32 a wave owns more
than 128 items, and the chunk-sum slots grow to 48 KiB of LDS — behind tables that differ from build to build.  The scalar-register
kernel and the plain resident kernel are held to the oracle over this axis elsewhere; here every OTHER instantiation is: the hierarchy
kernel (whole chunks, HALF, sm table), the five box builds, the pass builds and the adaptive builds, and the limits themselves.

Tolerance 0 everywhere — packed pixels and float mean as uint32, segments — against oracle.render, or tests/box_reference.render where
boxes are traced; never against another GPU frame.  Before a frame is rendered the CPU plan dump (tests/lds_plan.py) is asked which
build, tile and fold path the frame takes, with the host_frame value its entry point passes (render.hip: rt_hip_render and
rt_hip_render_progressive a page-locked frame; rt_hip_render_device into a tensor, and every adaptive pass, a frame in HBM), and the
test asserts it: a later change of tile policy cannot silently empty a case.  The last test prints, per build, every
(K, pixels_log2, fold path, HALF) the module's cases take.

The sweeps render 13 x 7: ragged against every tile shape (16 x 1 ... 4 x 1 page-locked, 8 x 4 ... 2 x 2 in HBM), and with most of them
the last workgroup of a row has waves without a tile.  Where the helpers of the progressive and adaptive tests are reused the frame is
their 37 x 23."""
import functools

import numpy as np
import pytest

import rt_amd
from oracle import binding as oracle
from rt_amd import capi
from tests import adaptive_reference as ref
from tests import box_bvh_cases as cases
from tests import box_reference as box_ref
from tests import lds_plan
from tests import test_gpu_adaptive as adaptive_tests
from tests import test_gpu_progressive as progressive_tests
from tests.test_gpu_boxes import boxes_scene, grid_spheres

pytestmark = pytest.mark.gpu

BVH = capi.RT_HIP_FLAG_BVH
DEVICE_BUILD = capi.RT_HIP_FLAG_BVH_DEVICE_BUILD
SM = capi.RT_HIP_FLAG_SM_MATERIALS
WHOLE = capi.RT_HIP_FLAG_FORCE_WHOLE_CHUNKS
RESIDENT = capi.RT_HIP_FLAG_FORCE_RESIDENT
BOXES = capi.RT_HIP_FLAG_TRACE_BOXES
TREE = BOXES | capi.RT_HIP_FLAG_BOX_BVH
UNSUPPORTED = 5
W, H = 13, 7
PW, PH = progressive_tests.W, progressive_tests.H  # 37 x 23
SEED = progressive_tests.SEED
PLANE = [(0, 1, 0, 0, 0)]
# What hipDeviceAttributeMaxSharedMemoryPerBlock says on the MI355X (the context plans with hipDeviceProp_t::sharedMemPerBlock, the same
# number): all of a compute unit's LDS.  OBSERVED, not derived; test_the_device_gives_a_workgroup_all_of_the_units_lds holds it.
DEVICE_LDS = 160 * 1024


# ---- the plan of a frame, and which build it names -------------------------------------------------------------------------------------
def camera_of(pod, width, height):
    return 0 if oracle.primary_ray(pod, width, height, 0, 0, want_form=True)[2] == "pinhole" else 2


def planned(pod, width, height, flags, host, spp=None, first=0, size=0, adaptive=0):
    """plan_launch as render.hip asks it for `pod`: `flags` are the call's, `host` the entry point's host_frame."""
    return lds_plan.plan(pod.n_spheres, pod.n_planes, width, height, pod.samples_per_pixel if spp is None else spp, n_boxes=pod.n_boxes, camera=camera_of(pod, width, height), flags=flags & ~DEVICE_BUILD, host_frame=host,
                         pass_first=first, pass_samples=size, adaptive=adaptive, lds_limit=DEVICE_LDS)


def build_name(p):
    """The instantiation of render_queue a plan names, as the kernel's comments call the builds."""
    if p["scan"] > 0:
        return f"scalar-register ({p['scan']} spheres, {p['planes']} planes)"
    scan = {0: "scan_resident", -4: "scan_bvh"}[p["scan"]]
    kind = "_adapt" if p["adaptive"] else "_pass" if p["pass"] else "_boxtree" if p["box_tree"] else "_boxes" if p["boxes"] else ""
    detail = [] if p["scan"] else ["scalar-load scan" if p["planes"] else "LDS scan, general camera" if p["general_camera"] else "LDS scan, pinhole"]
    detail.append("sm" if p["sm_table"] else "mg")
    return f"{scan}{kind} ({', '.join(detail)}{', HALF' if p['halves'] else ''})"


def cell(p):
    return (p["chunks"], p["pixels_log2"], lds_plan.fold_path(p), p["halves"])


def same_frame(got_rgba, got_rgb, want_rgba, want_rgb, what):
    assert np.array_equal(got_rgb.view(np.uint32), want_rgb.view(np.uint32)), f"{what}: float mean differs in {(got_rgb != want_rgb).any(axis=-1).sum()} of {want_rgba.size} pixels"
    assert np.array_equal(got_rgba, want_rgba), f"{what}: {(got_rgba != want_rgba).sum()} of {want_rgba.size} packed pixels differ"


def render_into_hbm(tracer, pod, width, height, seed, flags):
    """rt_hip_render_device of `pod` into tensors: (rgba8, float mean, stats)."""
    import torch

    tracer.upload(pod)
    frame = torch.full((height, width), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    mean = torch.full((height, width, 3), float("nan"), dtype=torch.float32, device="cuda:0")
    tracer.render_device(width, height, frame.data_ptr(), seed=seed, flags=flags, d_rgb_f32=mean.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return frame.cpu().numpy().view(np.uint32), mean.cpu().numpy(), tracer.stats()


def refused_and_nothing_launched(tracer, pod, width, height, flags, *words):
    """rt_hip_render refuses with RT_HIP_UNSUPPORTED and a message holding `words`; the canvas is untouched.  Returns the message."""
    canvas = np.full((height, width), 0xDEADBEEF, dtype=np.uint32)
    with pytest.raises(rt_amd.RtHipError) as refused:
        tracer.render(pod, width, height, seed=SEED, flags=flags, out=canvas)
    message = str(refused.value)
    assert refused.value.status == UNSUPPORTED and all(word in message for word in words), message
    assert (canvas == 0xDEADBEEF).all()
    return message


# ---- 1. the hierarchy kernel, one shot -------------------------------------------------------------------------------------------------
def field300(spp):
    return progressive_tests.field(300, 0, spp, 22, W, H)  # (progressive_tests.SCENES["field300_bvh"] at 13 x 7; sphere 0 is the ground)


@functools.lru_cache(maxsize=None)
def field300_reference(spp, sm):
    rgba, rgb, stats = oracle.render(field300(spp), W, H, seed=SEED, sm_materials=sm)
    rgba.setflags(write=False), rgb.setflags(write=False)
    return rgba, rgb, stats["segments"]


# spp: (K, pixels_log2 auto, pixels_log2 in whole chunks, HALF under auto); the last chunks hold 1, 1, 7, 16, 10, 16, 8 and 8 samples
HIERARCHY = {17: (2, 4, 5, 1), 33: (3, 3, 4, 1), 71: (5, 2, 3, 1), 144: (9, 2, 2, 1), 250: (16, 2, 2, 1), 272: (17, 2, 2, 0), 520: (33, 2, 2, 0), 1000: (63, 2, 2, 0)}
VARIANTS = {"auto": 0, "whole": WHOLE, "sm": SM}
ABOVE_64_KIB = [3409, 4096]  # 65 664 and 73 728 bytes of LDS: part 5


def hierarchy_plan(spp, variant, host):
    """The plan of the sweep's frame, held to the table above."""
    chunks, log2_auto, log2_whole, half = HIERARCHY.get(spp, (-(-spp // 16), 2, 2, 0))
    p = planned(field300(spp), W, H, BVH | VARIANTS[variant], host)
    auto = variant == "auto"
    assert (p["scan"], p["chunks"], p["pixels_log2"], p["sub_chunk_items"], p["sm_table"], p["refusal"]) == (-4, chunks, log2_auto if auto else log2_whole, half if auto else 0, int(variant == "sm"), ""), (spp, variant, p)
    assert (lds_plan.fold_path(p) == "channel-per-lane") == ((3 << p["pixels_log2"]) <= 64)
    return p


def check_hierarchy_frame(tracer, spp, variant, build=0):
    flags = BVH | VARIANTS[variant] | build
    pod = field300(spp)
    want_rgba, want_rgb, want_segments = field300_reference(spp, variant == "sm")
    hierarchy_plan(spp, variant, 1)
    rgba, rgb, stats = tracer.render(pod, W, H, seed=SEED, flags=flags, want_rgb=True)
    assert stats["kernel"] == "bvh" and stats["segments"] == want_segments, stats
    same_frame(rgba, rgb, want_rgba, want_rgb, f"rt_hip_render, {spp} spp, {variant}")
    hierarchy_plan(spp, variant, 0)
    rgba, rgb, stats = render_into_hbm(tracer, pod, W, H, SEED, flags)
    assert stats["kernel"] == "bvh" and stats["segments"] == want_segments, stats
    same_frame(rgba, rgb, want_rgba, want_rgb, f"rt_hip_render_device, {spp} spp, {variant}")


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("spp", list(HIERARCHY))
def test_the_hierarchy_kernel_one_shot(tracer, spp, variant):
    """scan_bvh in whole chunks, HALF (auto, up to K = 16) and under the sm table, into page-locked memory and into HBM."""
    check_hierarchy_frame(tracer, spp, variant)


def test_the_tables_tell_the_sweeps_scene_apart():
    """(what makes the sm frames a test of the sm build: the field has dielectric spheres)"""
    assert not np.array_equal(field300_reference(33, False)[0], field300_reference(33, True)[0])


@pytest.mark.parametrize("spp,variant", [(71, "auto"), (520, "sm")])
def test_the_hierarchy_kernel_on_the_device_built_tree(tracer, spp, variant):
    check_hierarchy_frame(tracer, spp, variant, DEVICE_BUILD)


# ---- 2. the box builds, one shot -------------------------------------------------------------------------------------------------------
def camera13():
    return cases.camera(W, H)


BOX_SCENES = {
    # name: (spp -> pod, flags, the kernel reported, (scan, planes, general_camera) of the build, the flag a refusal names)
    "boxes_pinhole": (lambda spp: boxes_scene((0.5, 1.6, 5.5), (0, 0, -1), spp).describe(W, H), BOXES, "resident", (0, 0, 0), "RT_HIP_FLAG_TRACE_BOXES"),
    "boxes_tilted": (lambda spp: boxes_scene((0.5, 1.6, 5.5), (0.3, -0.25, -1), spp).describe(W, H), BOXES, "resident", (0, 0, 1), "RT_HIP_FLAG_TRACE_BOXES"),
    "scalar_load": (lambda spp: box_ref.scene_pod(camera13(), spheres=grid_spheres(45), planes=PLANE, boxes=[(-1.5 + 0.7 * i, 0.3 + 0.1 * i, 0.8, 0.2, 0.3 + 0.1 * i, 0.2, i % 4) for i in range(5)], spp=spp), BOXES, "resident",
                    (0, 1, 0), "RT_HIP_FLAG_TRACE_BOXES"),
    "hierarchy_staged": (lambda spp: box_ref.scene_pod(camera13(), spheres=grid_spheres(200), planes=PLANE, boxes=[(-1.8 + 0.6 * i, 0.25 + 0.05 * i, 1.0, 0.2, 0.25 + 0.05 * i, 0.2, i % 4) for i in range(7)], spp=spp),
                         BOXES | BVH, "bvh", (-4, 0, 0), "RT_HIP_FLAG_TRACE_BOXES"),
    "box_tree": (lambda spp: cases.box_scene(cases.grid_boxes(300, pitch=0.3, half=0.1, z0=1.5), spheres=[(0, 0.6, 0, 0.5, 1)], planes=PLANE, spp=spp, size=(W, H)), TREE, "bvh", (-4, 0, 0), "RT_HIP_FLAG_BOX_BVH"),
}
BOX_SAMPLES = {33: (3, 4), 71: (5, 3), 144: (9, 2), 520: (33, 2)}  # spp: (K, pixels_log2): the channel-per-lane fold at three tile sizes, then more than 128 items per wave


@functools.lru_cache(maxsize=None)
def box_reference(name, spp, sm):
    rgba, rgb, stats = box_ref.render(BOX_SCENES[name][0](spp), W, H, seed=SEED, sm_materials=sm)
    rgba.setflags(write=False), rgb.setflags(write=False)
    return rgba, rgb, stats["segments"]


def box_plan(name, spp, table, host):
    make, flags, _, build, _ = BOX_SCENES[name]
    p = planned(make(spp), W, H, flags | table, host)
    if not p["refusal"]:
        assert (p["scan"], p["planes"], p["general_camera"], p["boxes"], p["box_tree"], p["sm_table"], p["sub_chunk_items"]) == (*build, 1, int(name == "box_tree"), int(bool(table)), 0), (name, spp, p)
    return p


@functools.lru_cache(maxsize=None)
def box_limits(name, table):
    """(the largest sample count the plan accepts, the first it refuses), from the dump: acceptance only ever ends once as the count grows."""
    low, high = 520, 8192
    assert not box_plan(name, low, table, 1)["refusal"] and box_plan(name, high, table, 1)["refusal"]
    while high - low > 1:
        middle = (low + high) // 2
        low, high = (low, middle) if box_plan(name, middle, table, 1)["refusal"] else (middle, high)
    assert all(bool(box_plan(name, spp, table, host)["refusal"]) == (spp == high) for spp in (low, high) for host in (0, 1))
    return low, high


@pytest.mark.parametrize("table", [0, SM], ids=["mg", "sm"])
@pytest.mark.parametrize("name", list(BOX_SCENES))
def test_the_box_builds(tracer, name, table):
    """33, 71, 144 and 520 samples, the first count the plan refuses — nothing is launched — and then the largest it accepts."""
    make, flags, kernel, _, flag_name = BOX_SCENES[name]
    flags |= table
    largest, first_refused = box_limits(name, table)
    tables = box_plan(name, largest, table, 1)["table_bytes"]
    if kernel == "resident":  # the slots' own limit: 4096 samples
        assert (largest, first_refused) == (4096, 4097)
    else:  # stacks (+ staged boxes) + 192 bytes per chunk reach 64 KiB
        assert largest % 16 == 0 and first_refused == largest + 1 and tables + 192 * (largest // 16) <= 65536 < tables + 192 * (largest // 16 + 1)
        assert tables == 24576 + (0 if name == "box_tree" else 32 * make(16).n_boxes)
    for spp in (*BOX_SAMPLES, first_refused, largest):
        pod = make(spp)
        if spp == first_refused:
            message = refused_and_nothing_launched(tracer, pod, W, H, flags, flag_name)
            assert box_plan(name, spp, table, 1)["refusal"] in message
            continue
        want_rgba, want_rgb, want_segments = box_reference(name, spp, bool(table))
        for host in (1, 0):
            p = box_plan(name, spp, table, host)
            assert (p["chunks"], p["pixels_log2"]) == BOX_SAMPLES.get(spp, (largest // 16, 2)) and p["refusal"] == "", (name, spp, p)
            rgba, rgb, stats = tracer.render(pod, W, H, seed=SEED, flags=flags, want_rgb=True) if host else render_into_hbm(tracer, pod, W, H, SEED, flags)
            assert stats["kernel"] == kernel and stats["segments"] == want_segments, (name, spp, host, stats)
            same_frame(rgba, rgb, want_rgba, want_rgb, f"{name}, {spp} spp, {'page-locked' if host else 'HBM'}")
    # the boxes are in the frame: without them (the oracle does not trace them) it is another one
    flat, _, _ = oracle.render(make(33), W, H, seed=SEED, want_rgb=False, sm_materials=bool(table))
    assert (box_reference(name, 33, bool(table))[0] != flat).mean() > 0.05


# ---- 3. the pass builds ----------------------------------------------------------------------------------------------------------------
PASS_SCENES = ["field300_bvh", "field1500", "basic_tilted", "field50", "dielectric_sm"]
# pass size: (the frame's samples: two whole passes and a short last one that ends inside a chunk, K, pixels_log2 of a whole pass)
PASS_SIZES = {80: (199, 5, 3), 144: (338, 9, 2), 528: (1156, 33, 2)}
MIXED = {"field300_bvh": (199, [16, 144, 0]), "field1500": (199, [16, 144, 0])}


def passes_of(spp, sizes):
    """[(first_sample, n_samples)] of run_passes(.., spp, sizes)."""
    out, done = [], 0
    while done < spp:
        size = sizes[min(len(out), len(sizes) - 1)]
        n = spp - done if size == 0 else min(-(-size // 16) * 16, spp - done)
        out.append((done, n))
        done += n
    return out


def pass_plans(name, spp, sizes):
    make, flags, _, build = progressive_tests.SCENES[name]
    pod = make(spp)
    plans = [planned(pod, PW, PH, flags, 1, first=first, size=n) for first, n in passes_of(spp, sizes)]
    for p, (first, n) in zip(plans, passes_of(spp, sizes)):
        assert (p["scan"], p["planes"], p["general_camera"], p["pass"], p["adaptive"], p["sub_chunk_items"], p["first_chunk"], p["chunks"], p["refusal"]) == (*build, 1, 0, 0, first // 16, -(-n // 16), ""), (name, p)
    return plans


def check_passes(tracer, name, spp, sizes):
    """run_passes holds every intermediate frame to the oracle; here: the final frame is rt_hip_render's and the segments add up."""
    make, flags, _, _ = progressive_tests.SCENES[name]
    rgba, rgb, stats = progressive_tests.run_passes(tracer, name, spp, sizes)
    assert [s["primary_samples"] // (PW * PH) for s in stats] == [n for _, n in passes_of(spp, sizes)]
    one_rgba, one_rgb, one_stats = tracer.render(make(spp), PW, PH, seed=SEED, flags=flags, want_rgb=True)
    same_frame(rgba, rgb, one_rgba, one_rgb, f"{name}: the last pass against rt_hip_render")
    assert sum(s["segments"] for s in stats) == one_stats["segments"] == progressive_tests.reference(name, spp)[2]


@pytest.mark.parametrize("size", list(PASS_SIZES))
@pytest.mark.parametrize("name", PASS_SCENES)
def test_passes_of_many_chunks(tracer, name, size):
    spp, chunks, pixels_log2 = PASS_SIZES[size]
    plans = pass_plans(name, spp, [size])
    assert len(plans) == 3 and [(p["chunks"], p["pixels_log2"]) for p in plans[:2]] == [(chunks, pixels_log2)] * 2 and plans[1]["first_chunk"] == chunks
    assert (spp - 2 * size) % 16 != 0 and 0 < spp - 2 * size < size  # the last pass is short and ends on a ragged chunk
    assert lds_plan.fold_path(plans[0]) == "channel-per-lane"
    check_passes(tracer, name, spp, [size])


@pytest.mark.parametrize("name", list(MIXED))
def test_mixed_pass_sizes_on_the_hierarchy(tracer, name):
    """16, then 144, then the rest: three tile shapes in one accumulation."""
    spp, sizes = MIXED[name]
    plans = pass_plans(name, spp, sizes)
    assert [(p["chunks"], p["pixels_log2"]) for p in plans] == [(1, 6), (9, 2), (3, 4)]
    check_passes(tracer, name, spp, sizes)


# ---- 4. the adaptive builds ------------------------------------------------------------------------------------------------------------
ADAPTIVE_SCENES = ["basic", "field300_bvh"]
ADAPTIVE_SIZES = {32: (2, 5), 80: (5, 3), 144: (9, 2)}  # pass size: (K, pixels_log2); a tile of 32 pixels folds per pixel, 8 and 4 fold one channel per lane
# min_samples = two passes; a threshold for which tests/adaptive_reference, run on the CPU over oracle frames at one and two passes, leaves
# between 294 and 666 of the 851 pixels stopped after the second pass on both scenes at all three sizes (0.03, the default, leaves 154 running
# at the worst; 0.08 only 9)
THRESHOLD = 0.02


def adaptive_params(size):
    return ref.params(min_samples=2 * size, threshold=THRESHOLD)


def adaptive_plan(name, size, first=0):
    make, flags, _, build = progressive_tests.SCENES[name]
    chunks, pixels_log2 = ADAPTIVE_SIZES[size]
    p = planned(make(3 * size), PW, PH, flags, 0, first=first, size=size, adaptive=1)
    assert (p["scan"], p["planes"], p["general_camera"], p["pass"], p["adaptive"], p["chunks"], p["pixels_log2"], p["first_chunk"], p["refusal"]) == (*build, 1, 1, chunks, pixels_log2, first // 16, ""), (name, size, p)
    return p


@pytest.mark.parametrize("size", list(ADAPTIVE_SIZES))
@pytest.mark.parametrize("name", ADAPTIVE_SCENES)
def test_the_promise_in_passes_of_many_chunks(tracer, name, size):
    """Three passes; after the second the map is mixed, so the third pass's waves hold stopped and running pixels side by side (with
    four-pixel tiles the stop mask has four live bits).  run_adaptive holds every pixel to the oracle at its own count after every pass."""
    for k in range(3):
        adaptive_plan(name, size, k * size)
    _, _, counts, stats, info = adaptive_tests.run_adaptive(tracer, name, 3 * size, size, adaptive_params(size))
    histogram = dict(zip(*np.unique(counts, return_counts=True)))
    print(f"{name}, passes of {size}: sample map {histogram}")
    assert info["passes"] == 3 and set(histogram) == {2 * size, 3 * size}, histogram
    assert (counts == 2 * size).sum() >= 100 and (counts == 3 * size).sum() >= 100, histogram
    assert stats[2]["primary_samples"] == int((counts == 3 * size).sum()) * size


@pytest.mark.parametrize("name", ADAPTIVE_SCENES)
def test_every_decision_in_passes_of_144_is_the_restatements(tracer, name):
    """rt_hip_adaptive_pass_device, three passes of nine chunks: state words and moments equal the CPU restatement replayed from the
    previous pass's words and this pass's own fold; a stopped pixel's words are never touched; the frame keeps the promise."""
    import torch

    size, pixels = 144, PW * PH
    make, flags, _, _ = progressive_tests.SCENES[name]
    p = adaptive_params(size)
    tracer.upload(make(3 * size))
    stream = torch.cuda.current_stream().cuda_stream
    block = torch.full((9 * pixels,), float("nan"), dtype=torch.float32, device="cuda:0")  # (the first pass must read none of it)
    frame = torch.zeros((PH, PW), dtype=torch.int32, device="cuda:0")
    mean = torch.zeros((PH, PW, 3), dtype=torch.float32, device="cuda:0")
    active = torch.full((1,), -1, dtype=torch.int32, device="cuda:0")
    nan_pattern = np.uint32(0x7FC0BEEF)

    def words():
        host = block.cpu().numpy().view(np.uint32)
        return host[: 3 * pixels].reshape(PH, PW, 3).copy(), host[3 * pixels : 4 * pixels].reshape(PH, PW).copy(), host[4 * pixels : 7 * pixels].reshape(PH, PW, 3).copy(), host[7 * pixels :].reshape(PH, PW, 2).copy()

    accum0 = state0 = moments0 = None
    for k in range(3):
        adaptive_plan(name, size, k * size)
        block[4 * pixels : 7 * pixels] = torch.from_numpy(np.full(3 * pixels, nan_pattern, dtype=np.uint32).view(np.float32)).to("cuda:0")  # the pass must rewrite what it traces
        tracer.adaptive_pass_device(PW, PH, size * k, size, block.data_ptr(), frame.data_ptr(), seed=SEED, flags=flags, params=p, d_rgb_f32=mean.data_ptr(), d_active_pixels=active.data_ptr(), stream=stream)
        torch.cuda.synchronize()
        accum, state, pass_sum, moments = words()
        was_stopped = np.zeros((PH, PW), dtype=bool) if k == 0 else (state0 & ref.STOPPED) != 0
        want_moments, want_state, want_rgba, want_rgb, want_active = ref.step(accum.view(np.float32), pass_sum.view(np.float32), np.zeros((PH, PW, 2), dtype=np.float32) if k == 0 else moments0.view(np.float32),
                                                                              np.zeros((PH, PW), dtype=np.uint32) if k == 0 else state0, size, k == 0, True, p)
        assert np.array_equal(state, want_state), f"pass {k}: {(state != want_state).sum()} state words differ from the restatement"
        assert np.array_equal(moments, want_moments.view(np.uint32)), f"pass {k}: moments differ from the restatement"
        assert int(active.cpu().numpy()[0]) == want_active == int(((state & ref.STOPPED) == 0).sum())
        got_rgba, got_rgb = frame.cpu().numpy().view(np.uint32), mean.cpu().numpy()
        same_frame(got_rgba, got_rgb, want_rgba, want_rgb, f"{name}, pass {k}: the frame against the restatement's")
        assert (pass_sum[~was_stopped] != nan_pattern).all()  # an active pixel: its pass sum was rewritten
        if k:  # a stopped pixel: neither read nor written
            assert (pass_sum[was_stopped] == nan_pattern).all() and np.array_equal(accum[was_stopped], accum0[was_stopped])
            assert np.array_equal(moments[was_stopped], moments0[was_stopped]) and np.array_equal(state[was_stopped], state0[was_stopped])
        else:
            assert np.array_equal(accum, pass_sum) and not np.isnan(accum.view(np.float32)).any()  # the running sum IS the first pass's fold
        counts = state & ref.COUNT
        adaptive_tests.assert_every_pixel_is_the_oracles_at_its_own_count(name, counts, got_rgba, got_rgb)
        if k == 1:  # the map is mixed: the third pass's four-pixel tiles hold stopped and running pixels side by side
            assert 100 <= int(((state & ref.STOPPED) != 0).sum()) <= pixels - 100, int(((state & ref.STOPPED) != 0).sum())
        accum0, state0, moments0 = accum, state, moments


# ---- 5. the limits ---------------------------------------------------------------------------------------------------------------------
def test_the_device_gives_a_workgroup_all_of_the_units_lds(tracer):
    """Read, nothing launched: 163 840 bytes.  Observed on the MI355X, not derived — every plan of this module is asked under it."""
    import torch

    assert torch.cuda.get_device_properties(0).shared_memory_per_block == DEVICE_LDS


def basic(spp, width=9, height=5):
    return rt_amd.Scene.named("basic").set_sampling(spp).describe(width, height)


@functools.lru_cache(maxsize=None)
def basic_reference(spp):
    rgba, rgb, stats = oracle.render(basic(spp), 9, 5, seed=SEED)
    rgba.setflags(write=False), rgb.setflags(write=False)
    return rgba, rgb, stats["segments"]


@pytest.mark.parametrize("flags,kernel", [(0, "small"), (RESIDENT, "resident")], ids=["scalar-register", "resident"])
def test_the_one_shot_limit_of_4096_samples(tracer, flags, kernel):
    """4081 (a last chunk of ONE sample) and 4096 are the oracle's frames; 4097 is refused, nothing is launched, the context renders on."""
    for spp in (4081, 4097, 4096):
        pod = basic(spp)
        if spp == 4097:
            refused_and_nothing_launched(tracer, pod, 9, 5, flags, "4097", "4096")
            tracer.upload(pod)
            import torch

            frame = torch.full((5, 9), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
            with pytest.raises(rt_amd.RtHipError) as refused:
                tracer.render_device(9, 5, frame.data_ptr(), seed=SEED, flags=flags, stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert refused.value.status == UNSUPPORTED and "4097" in str(refused.value) and bool((frame == 0x5A5A5A5A).all())
            continue
        want_rgba, want_rgb, want_segments = basic_reference(spp)
        for host in (1, 0):
            p = planned(pod, 9, 5, flags, host)
            assert (p["chunks"], p["pixels_log2"], p["slot_bytes"], p["halves"], p["refusal"]) == (256, 2, 48 * 1024, 0, "") and (p["scan"] == 0) == bool(flags), p
            rgba, rgb, stats = tracer.render(pod, 9, 5, seed=SEED, flags=flags, want_rgb=True) if host else render_into_hbm(tracer, pod, 9, 5, SEED, flags)
            assert stats["kernel"] == kernel and stats["segments"] == want_segments, stats
            same_frame(rgba, rgb, want_rgba, want_rgb, f"basic, {spp} spp, {'page-locked' if host else 'HBM'}")


def one_pass(tracer, pod, width, height, n, flags):
    """rt_hip_render_pass_device: samples [0, n) as one pass onto a NaN accumulator (the first pass reads none of it)."""
    import torch

    tracer.upload(pod)
    accum = torch.full((height, width, 3), float("nan"), dtype=torch.float32, device="cuda:0")
    frame = torch.full((height, width), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    mean = torch.zeros((height, width, 3), dtype=torch.float32, device="cuda:0")
    try:
        tracer.render_pass_device(width, height, 0, n, accum.data_ptr(), frame.data_ptr(), seed=SEED, flags=flags, d_rgb_f32=mean.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    finally:
        torch.cuda.synchronize()
    return frame.cpu().numpy().view(np.uint32), mean.cpu().numpy(), tracer.stats()


def test_the_limit_of_one_pass(tracer):
    """A pass of 4096 samples is the oracle's frame at 4096; a pass of 4112 is refused and says it is the pass."""
    p = planned(basic(4096), 9, 5, 0, 0, first=0, size=4096)
    assert (p["scan"], p["pass"], p["chunks"], p["slot_bytes"], p["refusal"]) == (0, 1, 256, 48 * 1024, "")
    rgba, rgb, stats = one_pass(tracer, basic(4096), 9, 5, 4096, 0)
    want_rgba, want_rgb, want_segments = basic_reference(4096)
    assert stats["kernel"] == "resident" and stats["segments"] == want_segments
    same_frame(rgba, rgb, want_rgba, want_rgb, "basic, one pass of 4096")
    with pytest.raises(rt_amd.RtHipError) as refused:
        one_pass(tracer, basic(4112), 9, 5, 4112, 0)
    assert refused.value.status == UNSUPPORTED and "a pass of 4112 samples" in str(refused.value)
    rgba, rgb, _ = tracer.render(basic(4096), 9, 5, seed=SEED, want_rgb=True)  # the context renders on
    same_frame(rgba, rgb, want_rgba, want_rgb, "basic after the refusal")


@pytest.mark.parametrize("variant", ["auto", "sm"])
@pytest.mark.parametrize("spp", ABOVE_64_KIB)
def test_the_hierarchy_kernel_above_64_kib_of_lds(tracer, spp, variant):
    """24 KiB of stacks and 192 bytes per chunk: 65 664 bytes at 3409 samples, 73 728 at 4096.  The MI355X gives a workgroup 160 KiB, the
    plan stands, and the frames are the oracle's (OBSERVED: no device refuses these at 64 KiB any more than this one does — that is
    tests/test_plan_lds_limit.py's, on the CPU)."""
    for host in (1, 0):
        assert hierarchy_plan(spp, variant, host)["lds_bytes"] == 24576 + 192 * -(-spp // 16) > 65536
    check_hierarchy_frame(tracer, spp, variant)


def test_one_pass_of_4096_samples_through_the_hierarchy(tracer):
    p = planned(field300(4096), W, H, BVH, 0, first=0, size=4096)
    assert (p["scan"], p["pass"], p["chunks"], p["pixels_log2"], p["lds_bytes"], p["refusal"]) == (-4, 1, 256, 2, 73728, "")
    rgba, rgb, stats = one_pass(tracer, field300(4096), W, H, 4096, BVH)
    want_rgba, want_rgb, want_segments = field300_reference(4096, False)
    assert stats["kernel"] == "bvh" and stats["segments"] == want_segments
    same_frame(rgba, rgb, want_rgba, want_rgb, "field300, one pass of 4096 through scan_bvh_pass")


def test_one_adaptive_pass_of_3424_samples_through_the_hierarchy(tracer):
    """The first adaptive pass stops nobody: the frame it leaves is the oracle's at 3424 samples."""
    import torch

    size = 3424
    p = planned(field300(size), W, H, BVH, 0, first=0, size=size, adaptive=1)
    assert (p["scan"], p["adaptive"], p["chunks"], p["pixels_log2"], p["lds_bytes"], p["refusal"]) == (-4, 1, 214, 2, 65664, "")
    tracer.upload(field300(size))
    block = torch.full((9 * W * H,), float("nan"), dtype=torch.float32, device="cuda:0")
    frame = torch.zeros((H, W), dtype=torch.int32, device="cuda:0")
    mean = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda:0")
    tracer.adaptive_pass_device(W, H, 0, size, block.data_ptr(), frame.data_ptr(), seed=SEED, flags=BVH, params=ref.params(min_samples=2 * size), d_rgb_f32=mean.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    want_rgba, want_rgb, want_segments = field300_reference(size, False)
    assert tracer.stats()["kernel"] == "bvh" and tracer.stats()["segments"] == want_segments
    same_frame(frame.cpu().numpy().view(np.uint32), mean.cpu().numpy(), want_rgba, want_rgb, "field300, one adaptive pass of 3424")
    state = block.cpu().numpy().view(np.uint32)[3 * W * H : 4 * W * H]
    assert (state == size).all()


# ---- what ran --------------------------------------------------------------------------------------------------------------------------
def test_every_build_is_swept_where_it_never_ran(capsys):
    """The cases above, asked of the plan dump once more: per build the (K, pixels_log2, fold path, HALF) its frames take.  Every build
    runs more than one chunk per pixel, the channel-per-lane fold and more than 128 items per wave; the HALF build its five tile shapes."""
    ran = {}

    def note(p):
        ran.setdefault(build_name(p), set()).add(cell(p))

    for spp in (*HIERARCHY, *ABOVE_64_KIB):
        for variant in VARIANTS:
            if spp in HIERARCHY or variant != "whole":
                for host in (1, 0):
                    note(hierarchy_plan(spp, variant, host))
    for name in BOX_SCENES:
        for table in (0, SM):
            for spp in (*BOX_SAMPLES, box_limits(name, table)[0]):
                note(box_plan(name, spp, table, 1))
    for name in PASS_SCENES:
        for size, (spp, _, _) in PASS_SIZES.items():
            for p in pass_plans(name, spp, [size]):
                note(p)
    for name, (spp, sizes) in MIXED.items():
        for p in pass_plans(name, spp, sizes):
            note(p)
    for name in ADAPTIVE_SCENES:
        for size in ADAPTIVE_SIZES:
            note(adaptive_plan(name, size, size))
    note(planned(field300(4096), W, H, BVH, 0, first=0, size=4096))
    note(planned(field300(3424), W, H, BVH, 0, first=0, size=3424, adaptive=1))
    with capsys.disabled():
        print("\nbuild: (K, pixels_log2, fold path, HALF) of the frames of tests/test_gpu_chunk_sweep.py")
        for build in sorted(ran):
            print(f"  {build}: " + ", ".join(f"({k}, {log2}, {fold}, {half})" for k, log2, fold, half in sorted(ran[build])))
    expected = ["scan_bvh (mg)", "scan_bvh (mg, HALF)", "scan_bvh (sm)", "scan_bvh_pass (mg)", "scan_bvh_adapt (mg)", "scan_bvh_boxes (mg)", "scan_bvh_boxes (sm)", "scan_bvh_boxtree (mg)", "scan_bvh_boxtree (sm)",
                "scan_resident_adapt (LDS scan, pinhole, mg)", "scan_resident_pass (LDS scan, general camera, mg)", "scan_resident_pass (scalar-load scan, mg)", "scan_resident_pass (LDS scan, pinhole, sm)"]
    expected += [f"scan_resident_boxes ({scan}, {table})" for scan in ("LDS scan, pinhole", "LDS scan, general camera", "scalar-load scan") for table in ("mg", "sm")]
    assert sorted(ran) == sorted(expected), sorted(ran)
    for build, cells in ran.items():
        if "HALF" in build:
            assert {(k, log2) for k, log2, _, _ in cells} == {(2, 4), (3, 3), (5, 2), (9, 2), (16, 2)}, (build, cells)
            continue
        assert any(k > 2 and fold == "channel-per-lane" and log2 == 2 for k, log2, fold, _ in cells), (build, cells)  # four pixels per wave
        assert any(k > 32 for k, *_ in cells) or "adapt (LDS" in build, (build, cells)  # more than 128 items per wave
        if "_adapt" in build:
            assert {5, 3, 2} <= {log2 for _, log2, _, _ in cells}, (build, cells)
        else:
            assert {4, 3, 2} <= {log2 for _, log2, _, _ in cells} or build == "scan_bvh (sm)" or "_pass" in build, (build, cells)
            assert any(fold == "per-pixel" and k > 1 for k, _, fold, _ in cells) or "_boxes" in build or "_boxtree" in build or "_pass" in build, (build, cells)
