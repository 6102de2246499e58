"""What the partition sweep shares (tests/test_partition_rows.py on the CPU, tests/test_gpu_partition_sweep.py on the GPU): the stripe
shapes, a row table written out as plain loops, one entry per build family of the render kernels with the CPU reference that holds
that build bit for bit, and the launch plan of every rank's share.  TEST INFRASTRUCTURE.

include/rt_hip.h promises that "the assembled image does not depend on `world`" for every build.  The code behind it is global_row's
three branches (world == 1, shift, division) called from separately written sites of kernels.hip — the tile set-up, the state reads,
both folds, the store, the rolling kernels' hand-out, preview_frame, assemble_stripes — and plan_launch is asked with the RANK's rows,
so a rank may take another tile shape than the whole frame.  SHAPES walks all of that at a frame height of 29: ragged against every
tile height, with stripes of 1, 2, 3, 5 and 7 rows under tiles of 8, 4 and 2, a last stripe that ends inside a tile, and ranks that
own nothing.

`row_table` is the reference of everything here.  It is NOT derived from rt_amd.distributed, frame_setup.hpp or the oracle:
tests/test_partition_rows.py ties each of those to it, and every CPU reference's `partition` argument too, so that the GPU tests need
one whole-frame reference render per (build, sample count) and pick each rank's rows out of it."""
import functools
from dataclasses import dataclass

import numpy as np

import rt_amd
from oracle import binding as oracle
from rt_amd import capi
from tests import box_bvh_cases
from tests import box_reference as box_ref
from tests import direct_reference as direct_ref
from tests import lds_plan
from tests import light_plan
from tests import light_reference as light_ref
from tests.bvh_cases import MATERIALS as FIELD_MATERIALS
from tests.bvh_cases import sphere_field
from tests.conftest import GOLDEN, PREVIEW_SCENE

FRAME = (37, 29)  # ragged against every tile width (16, 8, 4, 2) and height (8, 4, 2)
SMALL_FRAME = (5, 3)  # smaller than one tile of any shape
SEED = 29
DEVICE_LDS = 160 * 1024  # what the context plans under on the MI355X (tests/test_gpu_chunk_sweep.py holds the figure to the device)

# (world, stripe_rows) at a frame height of 29
SHAPES = [
    (1, 5),  # the whole image; a stripe value that must be ignored
    (2, 1),  # every tile row goes to another image row
    (4, 2),  # shift by 1
    (2, 8),  # shift; a ragged last stripe of 5 rows on rank 1
    (3, 5),  # division; the last stripe of 4 rows on rank 2
    (3, 7),  # division; the last stripe of ONE row on rank 1
    (5, 3),  # division; two stripes per rank, the last of 2 rows
    (2, 16),  # stripes of 16 and 13 rows
    (2, 32),  # a stripe taller than the frame: rank 1 owns nothing
    (7, 8),  # more ranks than stripes: ranks 4..6 own nothing
]
SMALL_SHAPES = [(2, 1), (2, 2), (3, 5)]  # at a frame height of 3
# plan_launch is asked with the rank's rows.  At 37 x 29 every share is planned as the whole frame is (choose_queue's thresholds are
# counts of pixels and items that no frame of that size reaches), so ONE frame is large enough to cross one: 1280 x 1024 at 17 samples is
# two chunks of 1 310 720 pixels = 5 x the lanes the device keeps resident, where a launch stops taking half chunks — the whole frame is
# cut into 8 x 4 tiles of whole chunks, every share of it into 4 x 4 tiles of half chunks (the oracle renders the frame in under a second)
LARGE_FRAME = (1280, 1024)
LARGE_SHAPES = [(1, 5), (2, 8), (3, 5)]
LARGE_CASE = ("small_auto", 17)


# ---- the row table -------------------------------------------------------------------------------------------------------------------
def row_table(height, world, stripe_rows):
    """(table, counts): table[y] = (rank, local row) of image row y, counts[rank] = rows of that rank.  include/rt_hip.h's rule
    spelled out: the image is cut from the top into stripes of `stripe_rows` rows, the last one as short as what is left; the stripes
    are dealt to the ranks in turn; a rank keeps its rows in the order it was dealt them."""
    assert height >= 0 and world >= 1 and stripe_rows >= 1
    table, counts = [], [0] * world
    y, stripe = 0, 0
    while y < height:
        rank = stripe % world
        taken = 0
        while taken < stripe_rows and y < height:
            table.append((rank, counts[rank]))
            counts[rank] += 1
            taken += 1
            y += 1
        stripe += 1
    return table, counts


def rows_of(height, world, stripe_rows, rank):
    """the image rows of `rank`, in the order of its local rows"""
    table, counts = row_table(height, world, stripe_rows)
    rows = [None] * counts[rank]
    for y in range(height):
        if table[y][0] == rank:
            rows[table[y][1]] = y
    return rows


def padded_rows(height, world, stripe_rows):
    return max(row_table(height, world, stripe_rows)[1])


def shapes_of(size):
    return {FRAME: SHAPES, SMALL_FRAME: SMALL_SHAPES, LARGE_FRAME: LARGE_SHAPES}[size]


# ---- scenes --------------------------------------------------------------------------------------------------------------------------
BVH = capi.RT_HIP_FLAG_BVH
DEVICE_BUILD = capi.RT_HIP_FLAG_BVH_DEVICE_BUILD
SM = capi.RT_HIP_FLAG_SM_MATERIALS
WHOLE = capi.RT_HIP_FLAG_FORCE_WHOLE_CHUNKS
HALF = capi.RT_HIP_FLAG_FORCE_HALF_CHUNKS
RESIDENT = capi.RT_HIP_FLAG_FORCE_RESIDENT
TILED = capi.RT_HIP_FLAG_FORCE_TILED
STREAMED = capi.RT_HIP_FLAG_FORCE_STREAMED
BOXES = capi.RT_HIP_FLAG_TRACE_BOXES
TREE = BOXES | capi.RT_HIP_FLAG_BOX_BVH
EMISSION = light_plan.EMISSION
DIRECT = light_plan.DIRECT
PREVIEW = capi.RT_HIP_FLAG_PREVIEW
TILTED = ((0.2, 1.2, 3.0), (0.3, -0.25, -1.0))  # (no pinhole at either frame size: the general-camera build; assert_build holds it)
PLANE = [(0, 1, 0, 0, 0)]
LAMBERT, METAL, DIELECTRIC = light_ref.LAMBERT, light_ref.METAL, light_ref.DIELECTRIC
LIGHT_MATERIALS = [(LAMBERT, (0.8, 0.8, 0.3), 0.0, 1.0), (METAL, (0.9, 0.6, 0.4), 0.2, 0.9), (DIELECTRIC, (0.9, 0.95, 1.0), 0.0, 1.5), (LAMBERT, (0.3, 0.5, 0.8), 0.0, 0.8), (LAMBERT, (0.5, 0.5, 0.5), 0.0, 1.0)]
LAMP = 4
LIGHT_TABLE = np.array([(0, 0, 0)] * 4 + [(4, 3.2, 2)], dtype=np.float32)
LIGHT_TABLE.setflags(write=False)
# a lamp, a lambert sphere, a metal sphere and a dielectric one over a plane (tests/test_gpu_light_chunk_sweep.py's small scene)
LIT_SPHERES = [(1.6, 2.6, -0.4, 0.6, LAMP), (-0.9, 0.7, -0.2, 0.7, 3), (0.9, 0.45, 0.6, 0.45, 1), (-0.1, 0.4, 1.6, 0.4, 2)]


def named(name, tilted=False):
    def make(spp, width, height):
        scene = rt_amd.Scene.named(name).set_sampling(spp)
        if tilted:
            scene.set_camera(*TILTED)
        return scene.describe(width, height)

    return make


def field(count, planes, seed):
    """`count` spheres (sphere 0 is the ground) seen from above: tests/test_gpu_progressive.py's fields at any frame size"""

    def make(spp, width, height):
        ivp = rt_amd.Scene.parse("").set_camera((0.0, 4.0, 3.0), (0.0, -0.35, -1.0)).describe(width, height).inverse_view_projection[:]
        return rt_amd.scene_from_arrays(sphere_field(np.random.default_rng(seed), count), [(0, 1, 0, 0.05, 2)] * planes, FIELD_MATERIALS, samples_per_pixel=spp, max_bounces=6, inverse_view_projection=ivp)

    return make


def boxes_toml(spp, width, height):
    return rt_amd.Scene.load(GOLDEN / "scenes" / "boxes.toml").set_sampling(spp).set_camera((0.5, 1.6, 5.5), (0, 0, -1)).describe(width, height)


def boxes_over_a_field(spp, width, height):
    """200 spheres, so that RT_HIP_FLAG_BVH's hierarchy has something to hold, and seven boxes staged into LDS behind its stacks"""
    boxes = [(-1.8 + 0.6 * i, 0.25 + 0.05 * i, 1.0, 0.2, 0.25 + 0.05 * i, 0.2, i % 4) for i in range(7)]
    return box_ref.scene_pod(box_bvh_cases.camera(width, height), spheres=light_ref.grid_spheres(200), planes=PLANE, boxes=boxes, spp=spp)


def box_tree(spp, width, height):
    return box_bvh_cases.box_scene(box_bvh_cases.grid_boxes(300, pitch=0.3, half=0.1, z0=1.5), spheres=[(0, 0.6, 0, 0.5, 1)], planes=PLANE, spp=spp, size=(width, height))


def light_camera(width, height):
    return rt_amd.Scene.parse("").set_camera((0.3, 1.5, 5.0), (0, 0, -1)).describe(width, height)


def lit_small(spp, width, height):
    return light_ref.scene_pod(light_camera(width, height), spheres=LIT_SPHERES, planes=PLANE, spp=spp, materials=LIGHT_MATERIALS)


def lit_field(spp, width, height):
    """300 spheres of which every sixtieth is a lamp, larger and lifted above the field: for the hierarchy"""
    spheres = [(x, 1.2, z + 2.0, 0.3, LAMP) if i % 60 == 7 else (x, y, z + 2.0, r, i % 4) for i, (x, y, z, r, _) in enumerate(light_ref.grid_spheres(300, radius=0.1, pitch=0.25))]
    return light_ref.scene_pod(light_camera(width, height), spheres=spheres, planes=PLANE, spp=spp, materials=LIGHT_MATERIALS)


def preview_scene(spp, width, height):
    return rt_amd.Scene.parse(PREVIEW_SCENE).set_sampling(spp).describe(width, height)


# ---- the builds ----------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Build:
    name: str
    family: str  # the row of the build table this entry belongs to
    make: object  # (spp, width, height) -> rt_hip_scene
    flags: int
    reference: str  # "oracle", "box", "light" or "direct": the CPU reference that holds this build bit for bit
    samples: tuple  # the frame's sample counts — a pass build's: (first pass, the frame's count)
    scan: tuple  # what the plan must say of a share with rows: (scan, planes, general_camera) — big-scene builds: (scan codes it may take,)
    tile_per_wave: bool = True  # the frame is cut into pixel tiles, one per wave (not the rolling kernels, not the preview)
    passes: bool = False  # through rt_hip_render_pass_device
    members: bool = False  # a multi-member context accepts the flag set: also rendered by direct-frame members

    @property
    def sm(self):
        return bool(self.flags & SM)

    @property
    def table(self):
        """the emission table the context is given, None for a build without lights"""
        return LIGHT_TABLE if self.reference in ("light", "direct") else None


FOUR = (5, 20, 40, 70)  # tiles of 8 rows at up to 16 samples, 4 rows at 17..64, 2 rows beyond (choose_queue, a frame in HBM)
THREE = (5, 20, 70)
PASSES = ((16, 21), (32, 52), (16, 86))  # one chunk then 5 samples; two chunks then 20 samples; one chunk then 70 samples: tiles of 8, 4 and 2 rows
BUILDS = [
    # the scalar-register kernel: by the size of the launch, whole chunks, half chunks
    Build("small_auto", "scalar-register", named("basic"), 0, "oracle", FOUR, (None, None, 0)),
    Build("small_whole", "scalar-register", named("basic"), WHOLE, "oracle", FOUR, (None, None, 0)),
    Build("small_half", "scalar-register", named("basic"), HALF, "oracle", FOUR, (None, None, 0)),
    # the resident kernel: the LDS scan through a pinhole and a general camera, the scalar-load scan, both tables
    Build("resident_pinhole", "resident", named("basic"), RESIDENT, "oracle", FOUR, (0, 0, 0), members=True),
    Build("resident_general", "resident", named("basic", tilted=True), RESIDENT, "oracle", THREE, (0, 0, 1)),
    Build("resident_scalar_load", "resident", field(50, 1, 21), RESIDENT, "oracle", THREE, (0, 1, 0)),
    Build("resident_sm", "resident", named("dielectric"), RESIDENT | SM, "oracle", THREE, (0, 0, 0), members=True),
    Build("resident_scalar_load_sm", "resident", field(50, 1, 21), RESIDENT | SM, "oracle", THREE, (0, 1, 0)),
    # the rolling kernels on a field of 1500 spheres, at low sample counts
    Build("tiled", "tiled, streamed", field(1500, 0, 23), TILED, "oracle", (2, 20), ((-1,),), tile_per_wave=False),
    Build("streamed", "tiled, streamed", field(1500, 0, 23), STREAMED, "oracle", (2, 20), ((-2, -3),), tile_per_wave=False),
    # the hierarchy kernel on both builders, both tables
    Build("bvh_mg", "hierarchy", field(300, 0, 22), BVH, "oracle", FOUR, (-4, 0, 0), members=True),
    Build("bvh_sm", "hierarchy", field(300, 0, 22), BVH | SM, "oracle", THREE, (-4, 0, 0)),
    Build("bvh_device_mg", "hierarchy", field(300, 0, 22), BVH | DEVICE_BUILD, "oracle", THREE, (-4, 0, 0), members=True),
    Build("bvh_device_sm", "hierarchy", field(300, 0, 22), BVH | DEVICE_BUILD | SM, "oracle", THREE, (-4, 0, 0)),
    # the box builds
    Build("boxes_resident", "boxes", boxes_toml, BOXES, "box", THREE, (0, 0, 0), members=True),
    Build("boxes_bvh", "boxes", boxes_over_a_field, BOXES | BVH, "box", THREE, (-4, 0, 0), members=True),
    Build("boxes_tree", "boxes", box_tree, TREE, "box", THREE, (-4, 0, 0), members=True),
    # the light and the direct-light builds, resident and hierarchy
    Build("lights_resident", "lights", lit_small, EMISSION, "light", THREE, (0, 0, 0), members=True),
    Build("lights_bvh", "lights", lit_field, EMISSION | BVH, "light", THREE, (-4, 0, 0)),
    Build("direct_resident", "lights", lit_small, DIRECT, "direct", THREE, (0, 0, 0), members=True),
    Build("direct_bvh", "lights", lit_field, DIRECT | BVH, "direct", THREE, (-4, 0, 0)),
    # the pass builds
    Build("pass_resident", "passes", named("basic"), 0, "oracle", PASSES, (0, 0, 0), passes=True),
    Build("pass_bvh", "passes", field(300, 0, 22), BVH, "oracle", PASSES, (-4, 0, 0), passes=True),
    # the preview, with boxes in the scene
    Build("preview", "preview", preview_scene, PREVIEW, "oracle", (1,), (), tile_per_wave=False),
]
BY_NAME = {build.name: build for build in BUILDS}
FAMILIES = ["scalar-register", "resident", "tiled, streamed", "hierarchy", "boxes", "lights", "passes", "preview"]
CASES = [(build.name, samples) for build in BUILDS for samples in build.samples]  # one GPU test each


def case_id(name, samples):
    return f"{name}-{samples[0]}+{samples[1] - samples[0]}" if isinstance(samples, tuple) else f"{name}-{samples}spp"


def total_of(samples):
    """the frame's sample count"""
    return samples[1] if isinstance(samples, tuple) else samples


def small_frame_samples(build):
    """the one sample count a build renders the 5 x 3 frame at: its second (two chunks), or its only one"""
    return build.samples[min(1, len(build.samples) - 1)]


@functools.lru_cache(maxsize=None)
def pod_of(name, spp, size):
    return BY_NAME[name].make(spp, *size)


# ---- the references ------------------------------------------------------------------------------------------------------------------
def reference_render(name, spp, size, partition=None):
    """The build's CPU reference: (rgba, float mean, stats dict) of the whole frame, or of `partition`'s rows as the reference cuts them"""
    build = BY_NAME[name]
    pod = pod_of(name, spp, size)
    if build.reference == "oracle":
        return oracle.render(pod, *size, seed=SEED, partition=partition, sm_materials=build.sm, preview=bool(build.flags & PREVIEW))
    if build.reference == "box":
        return box_ref.render(pod, *size, seed=SEED, partition=partition, sm_materials=build.sm)
    render = direct_ref.render if build.reference == "direct" else light_ref.render
    return render(pod, *size, LIGHT_TABLE, seed=SEED, partition=partition, sm_materials=build.sm)


@functools.lru_cache(maxsize=None)
def reference(name, spp, size=FRAME):
    """(rgba, float mean, segments) of the whole frame: computed once, shared, read-only"""
    rgba, rgb, stats = reference_render(name, spp, size)
    rgba.setflags(write=False), rgb.setflags(write=False)
    return rgba, rgb, stats["segments"]


# ---- the plans -----------------------------------------------------------------------------------------------------------------------
def camera_of(pod, size):
    return 0 if oracle.primary_ray(pod, *size, 0, 0, want_form=True)[2] == "pinhole" else 2


@functools.lru_cache(maxsize=None)
def plan(name, samples, size, local_rows):
    """plan_launch as rt_hip_render_device asks it for a share of `local_rows` rows of a one-shot frame in HBM (the builder's flag is
    taken out of the launch's, as check_render_request does).  None for the preview, which is not planned."""
    build = BY_NAME[name]
    assert not build.passes
    if build.flags & PREVIEW:
        return None
    pod = pod_of(name, samples, size)
    flags = build.flags & ~DEVICE_BUILD
    if build.table is not None:
        lights, sampled = light_plan.light_counts(pod, LIGHT_TABLE)
        return dict(light_plan.ask((pod.n_spheres, pod.n_planes, size[0], local_rows, samples, camera_of(pod, size), flags, 0, lights, sampled, DEVICE_LDS)))
    return lds_plan.plan(pod.n_spheres, pod.n_planes, size[0], local_rows, samples, n_boxes=pod.n_boxes, camera=camera_of(pod, size), flags=flags, host_frame=0, lds_limit=DEVICE_LDS)


def pass_windows(samples):
    """[(first sample, the frame's count after the pass)] of a pass build's case"""
    first, total = samples
    return [(0, first), (first, total)]


def plans_of(name, samples, size, local_rows):
    """the plans of every launch the case makes for such a share: one, or one per pass"""
    build = BY_NAME[name]
    if not build.passes:
        return [plan(name, samples, size, local_rows)]
    # (a pass is planned with the scene's sample count — the frame's — and its own window)
    return [_pass_plan(name, samples[1], size, local_rows, first, after - first) for first, after in pass_windows(samples)]


@functools.lru_cache(maxsize=None)
def _pass_plan(name, total, size, local_rows, first, n):
    build = BY_NAME[name]
    pod = pod_of(name, total, size)
    return lds_plan.plan(pod.n_spheres, pod.n_planes, size[0], local_rows, total, n_boxes=pod.n_boxes, camera=camera_of(pod, size), flags=build.flags & ~DEVICE_BUILD, host_frame=0, pass_first=first, pass_samples=n, lds_limit=DEVICE_LDS)


def tile_height(p):
    return 1 << (p["pixels_log2"] - p["tile_w_log2"])


def assert_build(name, p, local_rows):
    """the share takes the build its entry names, or nothing where it has no rows: a change of policy cannot silently empty a case"""
    build = BY_NAME[name]
    assert p["refusal"] == "", (name, local_rows, p)
    assert (p["variant"] != 0) == (local_rows != 0), (name, local_rows, p)  # (RT_HIP_KERNEL_NONE: nothing is launched)
    if not build.tile_per_wave:
        assert p["big_scene"] == 1 and p["scan"] in build.scan[0], (name, p)
        return
    assert p["big_scene"] == 0 and p["pass"] == int(build.passes), (name, p)
    if build.family == "scalar-register":
        assert p["scan"] > 0 and p["general_camera"] == 0, (name, p)
    else:
        assert (p["scan"], p["planes"], p["general_camera"]) == build.scan, (name, p)
    assert p["sm_table"] == int(build.sm), (name, p)
    if build.family == "boxes":
        assert p["boxes"] == 1 and p["box_tree"] == int(build.flags & capi.RT_HIP_FLAG_BOX_BVH != 0), (name, p)
    if build.family == "lights":
        assert p["lights"] == 1 and p["direct"] == int(build.reference == "direct"), (name, p)


def cases_at(size):
    """[(build name, samples)] the sweep renders at `size`: every case at 37 x 29, every build once at 5 x 3, one case at 1280 x 1024"""
    if size == FRAME:
        return list(CASES)
    return [(build.name, small_frame_samples(build)) for build in BUILDS] if size == SMALL_FRAME else [LARGE_CASE]


def every_share(size=FRAME):
    """(build, samples, (world, stripe_rows), rank, local_rows) of every launch of the sweep at `size`"""
    for name, samples in cases_at(size):
        for world, stripe in shapes_of(size):
            counts = row_table(size[1], world, stripe)[1]
            for rank in range(world):
                yield BY_NAME[name], samples, (world, stripe), rank, counts[rank]
