"""Every frame the API accepts plans a launch grid that is in range (rt_amd/csrc/launch_plan.cpp), on the CPU.

tests/test_launch_plan.py pins the policy on frames up to 3840 x 2160.  The frames here are the other end: one pixel wide and 131070 rows
high, one row high and 8M pixels wide, one row past a whole tile at 70000 rows, the 2^32 - 1 pixels of 65535 x 65537.  check_render_request
accepts every one of them (asserted through box_plan_dump, which asks it first), so every one must plan a launch the device takes: at most
65535 workgroups in y (the code's own bound: the device's is not asked), at least one and at most 2^31 - 1 in x, tiles that cover the frame
without a whole spare tile row or column, and an item count that is the frame's in 64 bits.

The one way this went wrong: a page-locked host frame takes tiles "as wide as the tile allows", from 64 samples a pixel upwards ONE row
high, and a frame of more than 65535 rows then asked for as many workgroups in y.  plan_launch now takes the next taller shape of the same
pixel count there (cut_tiles); test_host_frames_of_many_rows_take_the_next_taller_tile pins that rule and that nothing else moved.

The other plan fixtures' request shapes — a pass, an adaptive pass, traced boxes with and without their tree, lights, direct light — go through
the dump programs their own tests use (tests/extreme_shapes.py builds them the same way)."""
import itertools

import pytest

from rt_amd import capi
from tests import adaptive_plan, extreme_shapes, pass_plan
from tests.test_launch_plan import FLAGS, KERNEL, row_invariants

pytestmark = pytest.mark.skipif(not extreme_shapes.have_compiler(), reason="no g++")

SHAPES = [(1, 1), (1, 65535), (1, 65536), (3, 65537), (3, 70001), (5, 32768), (5, 32769), (1, 131070), (16, 131070), (70001, 1), (65537, 3), (262145, 1), (8388608, 1), (65535, 65537)]
SAMPLES = [1, 16, 17, 20, 64, 256, 1000, 4096]
HOST = [0, 1]
CAMERAS = [0, 1, 2]  # camera_form: pinhole, plain eye form, other
SCENES = [(4, 0), (8, 0), (5, 3), (0, 1), (40, 0), (700, 2), (1500, 0), (100000, 0)]
MAX_GRID_Y = 65535
MAX_GRID_X = 0x7FFFFFFF
SAMPLE_CHUNK = 16


def request(scene, shape, spp, camera, flags, host):
    return (scene[0], scene[1], 1, shape[0], shape[1], spp, camera, flags, host, 1 if flags & capi.RT_HIP_FLAG_FAST else 0)


def requests():
    """the whole cross product: 14 shapes x 8 sample counts x 2 destinations x 3 cameras x 8 scenes x 9 flag words"""
    return [request(scene, shape, spp, camera, flags, host) for shape, spp, host, camera, scene, flags in itertools.product(SHAPES, SAMPLES, HOST, CAMERAS, SCENES, FLAGS)]


def grid_faults(r, items_per_pixel=None):
    """What is wrong with one plan's grid and tiles, as a list of words: `r` has width, local_rows, pixels_log2, tile_w_log2, tiles_x, tiles_y,
    grid_x, grid_y and, where items_per_pixel is given, total_items."""
    faults = []
    tile_w_log2, tile_h_log2 = r["tile_w_log2"], r["pixels_log2"] - r["tile_w_log2"]
    if r["grid_y"] > MAX_GRID_Y:
        faults.append(f"grid_y {r['grid_y']} > {MAX_GRID_Y}")
    if not 1 <= r["grid_x"] <= MAX_GRID_X:
        faults.append(f"grid_x {r['grid_x']} outside 1..{MAX_GRID_X}")
    if tile_h_log2 < 0 or (r["tiles_x"] << tile_w_log2) < r["width"] or (r["tiles_y"] << tile_h_log2) < r["local_rows"]:
        faults.append("the tiles do not cover the frame")
    elif ((r["tiles_x"] - 1) << tile_w_log2) >= r["width"] or ((r["tiles_y"] - 1) << tile_h_log2) >= r["local_rows"]:
        faults.append("a whole spare tile row or column")
    if items_per_pixel is not None and r["total_items"] != r["width"] * r["local_rows"] * items_per_pixel:  # (Python's integers: no 32-bit wrap on this side)
        faults.append(f"total_items {r['total_items']} is not {r['width']} x {r['local_rows']} x {items_per_pixel}")
    return faults


def items_per_pixel(r):
    """the rolling kernels' sub-chunk items: ceil(samples / item_samples); every other launch: one item per chunk of 16 samples"""
    chunks = (r["samples_per_pixel"] + SAMPLE_CHUNK - 1) // SAMPLE_CHUNK
    assert r["chunks"] == chunks, r
    if r["big_scene"] and r["halves"]:
        return (r["samples_per_pixel"] + r["item_samples"] - 1) // r["item_samples"]
    return chunks


@pytest.fixture(scope="module")
def rows():
    return extreme_shapes.table_rows(requests())


def test_every_accepted_frame_plans_a_grid_in_range(rows):
    assert len(rows) == len(SHAPES) * len(SAMPLES) * len(HOST) * len(CAMERAS) * len(SCENES) * len(FLAGS)
    failing = []
    for r in rows:
        faults = grid_faults(r, items_per_pixel(r))
        if faults:
            failing.append((tuple(r[k] for k in ("n_spheres", "n_planes", "planes_tame", "width", "local_rows", "samples_per_pixel", "camera", "flags", "host_frame", "fast_arithmetic")), r["pixels_log2"], r["tile_w_log2"], r["grid_x"], r["grid_y"], faults))
    text = "".join(f"\n request {' '.join(str(v) for v in req)}: pixels_log2 {p} tile_w_log2 {w} grid {gx} x {gy}: {'; '.join(faults)}" for req, p, w, gx, gy, faults in failing[:40])
    assert not failing, f"{len(failing)} of {len(rows)} plans are out of range; the first of them:{text}"


def test_the_invariants_the_kernels_rely_on_hold_at_the_extremes(rows):
    seen = set()
    for r in rows:
        row_invariants(r)
        seen.add(r["variant"])
    assert seen == {KERNEL["resident"], KERNEL["tiled"], KERNEL["small"], KERNEL["streamed"], KERNEL["bvh"]}


def test_host_frames_of_many_rows_take_the_next_taller_tile(rows):
    """The rule (launch_plan.cpp, cut_tiles), restated: a tile-per-wave plan whose widest-row shape would give more than 65535 tile rows takes
    tile_w_log2 one lower — tiles of the same pixel count, two rows high — and every other plan has the shape choose_queue always gave it: the
    device frame's (pixels_log2 + 1) / 2, the host frame's min(pixels_log2, 4) or its one 8 x 2 exception.  Both kinds of row occur."""
    taller = 0
    for r in rows:
        if r["big_scene"]:
            assert (r["pixels_log2"], r["tile_w_log2"], r["grid_y"]) == (0, 0, 1), r
            continue
        if not r["host_frame"]:
            assert r["tile_w_log2"] == (r["pixels_log2"] + 1) // 2, r
            continue
        widest = min(r["pixels_log2"], 4)
        if not r["halves"] and r["pixels_log2"] == 4 and r["chunks"] == 16 and r["n_spheres"] + r["n_planes"] < 5:
            widest = 3
        one_row_high = r["pixels_log2"] == widest
        if one_row_high and r["local_rows"] > MAX_GRID_Y:
            assert r["tile_w_log2"] == widest - 1 and r["tiles_y"] == (r["local_rows"] + 1) // 2, r
            taller += 1
        else:
            assert r["tile_w_log2"] == widest, r
    assert taller


# ---- the other plan fixtures' request shapes ----------------------------------------------------------------------------------------------
BOXES = capi.RT_HIP_FLAG_TRACE_BOXES
TREE = BOXES | capi.RT_HIP_FLAG_BOX_BVH
EMISSION = capi.RT_HIP_FLAG_EMISSION
DIRECT = EMISSION | capi.RT_HIP_FLAG_DIRECT_LIGHT
SM = capi.RT_HIP_FLAG_SM_MATERIALS
BVH = capi.RT_HIP_FLAG_BVH
FAMILY_SCENES = [(4, 1), (45, 1), (1500, 0)]  # the LDS scan, the scalar-load scan, the hierarchy


def check_family(name, asked, answers, chunked_by):
    """every answer is a plan in range, or a refusal by the PLAN (LDS, chunk sums): never one of the frame's shape, which the API accepts"""
    planned = set()
    for (shape, spp, host), answer in zip(asked, answers):
        if isinstance(answer, str):
            assert answer.startswith("refused 5 ") and ("LDS" in answer or "chunk sums" in answer), (name, shape, spp, host, answer)
            continue
        r = dict(answer, width=shape[0], local_rows=shape[1])
        assert not r.get("big_scene", 0), (name, shape, spp, host)
        assert r["chunks"] == (chunked_by(spp) + SAMPLE_CHUNK - 1) // SAMPLE_CHUNK, (name, shape, spp, host, r)
        faults = grid_faults(r, r["chunks"] if "total_items" in r else None)
        assert not faults, (name, shape, spp, host, faults, r)
        assert (r["grid_x"], r["grid_y"]) == ((r["tiles_x"] + 3) // 4, r["tiles_y"]), (name, shape, spp, host, r)
        planned.add((shape, host))
    assert planned == {(shape, host) for shape, _, host in asked}, name  # no shape is only ever refused


def test_passes_of_progressive_frames():
    """a pass of `spp` samples of a 4096-sample frame, the second pass of its size (tests/pass_plan.py)"""
    for scene in FAMILY_SCENES:
        for flags in (0, SM, BVH):
            asked = [(shape, spp, host) for shape in SHAPES for spp in SAMPLES for host in HOST]
            answers = pass_plan.plans([(scene[0], scene[1], 1, shape[0], shape[1], 8192, 0, flags, host, 0, 2 * SAMPLE_CHUNK * ((spp + SAMPLE_CHUNK - 1) // SAMPLE_CHUNK), spp) for shape, spp, host in asked])
            for a in answers:
                assert a["pass"] == 1
            check_family(f"pass {scene} {flags}", asked, answers, lambda spp: spp)


def test_adaptive_passes():
    """adaptive passes go into the context's own buffers: no host frame (tests/adaptive_plan.py asks for none)"""
    for scene in FAMILY_SCENES:
        for flags in (0, SM, BVH):
            asked = [(shape, spp, 0) for shape in SHAPES for spp in SAMPLES]
            answers = adaptive_plan.plans([(scene[0], scene[1], 1, shape[0], shape[1], 8192, 0, flags, 2 * SAMPLE_CHUNK * ((spp + SAMPLE_CHUNK - 1) // SAMPLE_CHUNK), spp) for shape, spp, _ in asked])
            for a in answers:
                assert a["adaptive"] == 1 and a["pixels_log2"] <= 6
            check_family(f"adaptive {scene} {flags}", asked, answers, lambda spp: spp)


@pytest.mark.parametrize("flags", [BOXES, BOXES | SM, TREE, TREE | SM, BOXES | BVH], ids=["boxes", "boxes_sm", "box_tree", "box_tree_sm", "boxes_bvh"])
def test_traced_boxes(flags):
    for scene in FAMILY_SCENES:
        for camera in (0, 2):
            asked = [(shape, spp, host) for shape in SHAPES for spp in SAMPLES for host in HOST]
            answers = extreme_shapes.named_rows("box_plan_dump", [(scene[0], scene[1], 3, shape[0], shape[1], spp, camera, flags, host) for shape, spp, host in asked])
            for a in answers:
                assert isinstance(a, str) or a["boxes"] == 1
            check_family(f"boxes {scene} {flags}", asked, answers, lambda spp: spp)


@pytest.mark.parametrize("dumper,flags", [("light_plan_dump", EMISSION), ("light_plan_dump", EMISSION | SM), ("light_plan_dump", EMISSION | BVH), ("direct_plan_dump", DIRECT), ("direct_plan_dump", DIRECT | SM), ("direct_plan_dump", DIRECT | BVH)],
                         ids=["lights", "lights_sm", "lights_bvh", "direct", "direct_sm", "direct_bvh"])
def test_lights_and_direct_light(dumper, flags):
    tail = (5, 1, 5) if dumper == "light_plan_dump" else (5, 1, 5, 1)  # table_rows n_lights scene_materials [n_sampled_lights]
    for scene in FAMILY_SCENES:
        for camera in (0, 2):
            asked = [(shape, spp, host) for shape in SHAPES for spp in SAMPLES for host in HOST]
            answers = extreme_shapes.named_rows(dumper, [(scene[0], scene[1], shape[0], shape[1], spp, camera, flags, host, *tail) for shape, spp, host in asked])
            for a in answers:
                assert isinstance(a, str) or (a["lights"] == 1 and a.get("direct", 0) == (1 if dumper == "direct_plan_dump" else 0))
            check_family(f"{dumper} {scene} {flags}", asked, answers, lambda spp: spp)


def test_one_row_past_the_height_the_api_accepts_is_refused():
    """the frames above are accepted; 131071 rows are not, by name, before anything is planned"""
    accepted, refused = extreme_shapes.named_rows("box_plan_dump", [(4, 0, 0, 1, 131070, 64, 0, 0, 1), (4, 0, 0, 1, 131071, 64, 0, 0, 1)])
    assert isinstance(accepted, dict) and accepted["grid_y"] == 65535
    assert refused == "refused 1 rt_hip_render_device: frame height 131071 exceeds the supported 131070 rows"


# ---- the case table of tests/test_gpu_extreme_shapes.py -------------------------------------------------------------------------------------
def test_the_gpu_tests_frames_take_the_kernels_and_tiles_their_table_records():
    assert set(extreme_shapes.EXPECTED) == set(extreme_shapes.ONE_SHOT)
    for case in extreme_shapes.ONE_SHOT:
        for host in (1, 0):
            p = extreme_shapes.plan(*case, host)
            assert p["refusal"] == "" and not grid_faults(dict(p, width=case[2][0], local_rows=case[2][1])), (case, host, p)
            assert extreme_shapes.tile_of(p) == extreme_shapes.EXPECTED[case][1 - host], (case, host, p)
    # the families reach every kernel, whole and half chunks, and tiles 1, 2, 4 and 8 rows high; the host frames beyond 65535 rows two-row tiles only
    tiles = {tile for pair in extreme_shapes.EXPECTED.values() for tile in pair}
    assert {kernel for kernel, _, _ in tiles} == {"small", "resident", "bvh", "tiled", "streamed"} and {h for _, _, h in tiles} == {0, 1, 2, 4, 8}
    assert all(extreme_shapes.EXPECTED[case][0][2] in (0, 2) for case in extreme_shapes.ONE_SHOT if case[2][1] > MAX_GRID_Y)  # (0: the rolling kernels)
    assert {extreme_shapes.plan(*case, 1)["halves"] for case in extreme_shapes.ONE_SHOT} == {0, 1}


@pytest.mark.parametrize("case", [c for c in extreme_shapes.ONE_SHOT if c[0] in ("small_auto", "resident_general", "tiled")], ids=lambda c: extreme_shapes.case_id(*c))
def test_the_stretched_frames_show_sky_and_scene(case):
    """The camera of a 96 x 54 frame over the extreme shape: not a frame of sky alone (a kernel that placed every tile wrongly would still be
    right), not one of ground alone.  A frame one row high is the camera's horizon row — no sky to ask for."""
    name, spp, size = case
    differs = extreme_shapes.reference(name, spp, size)[0] != extreme_shapes.sky_only(name, spp, size)
    assert differs.mean() >= 0.05, (case, differs.mean())
    if size[1] > 1:
        assert 1.0 - differs.mean() >= 0.05, (case, differs.mean())
