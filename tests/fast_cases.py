"""The frames RT_HIP_FLAG_FAST's builds are held to per pixel (tests/fast_reference.py has the rule), and the plan each must take.

CONSTANTS.  A = 64 ulps and R = 32 runs make the ensemble; the stand-ins for a FAST frame (tests/test_fast_reference.py) are single
perturbed runs at S = 4 and S / 2 ulps; the allowance is 2e-5 * scale + 2 * spread.  S is tied to the device by
tests/test_gpu_fast_math.py, which holds the measured error of v_sqrt / v_rcp / v_rsq and of divide() to S / 2 ulps: were a leaf error
above 2 ulps ever measured, S becomes twice it rounded up to a power of two and A grows by the same factor — the allowance is not widened
by hand.

SCENES.  Unit-scale spheres over a floor, at most a back wall and a side wall (random walls leave the rule few pixels with teeth), no
radius-1000 ground (its self-intersection margin is about 8 ulps: every bounce off it is a coin toss).  Materials are lambert or metal
(FAST is mg-only) with albedo channels in [0.5, 1] and albedo x reflectivity <= 1, and at most 6 bounces: every channel of a pixel's mean
is then at least 0.5^7 of its largest (each bounce and the sky keep the ratio above 1/2; a path that ends black is black in all three) —
what the packed-pixel bound of tests/test_fast_reference.py rests on.

SWEEPS.
  builds   37 x 23 (ragged against 16 x 1 ... 4 x 1 and 8 x 4 ... 2 x 2 tiles): all 26 (spheres, planes) pairs of the scalar-register
           kernel x {pinhole, eye: a tilted camera whose matrix has rounding noise in w's x / y terms} x {whole chunks, HALF}; the two item
           forms share the reference.  12, 23 or 25 samples: HALF's second half is ragged (4, 7 and 1 samples in the last item).
  chunks   13 x 7, 17 ... 520 samples: K = 2 ... 33 across the pixels_log2 and fold-path changes; one scalar-register build and the forced
           resident kernel, whole and auto (auto is HALF up to K = 16), all four sharing one reference per sample count.
  kernels  37 x 23: the three resident forms (pinhole; general camera through an orthographic matrix; the scalar-load scan, from 40
           spheres, with a plane), tiled and streamed, each in whole chunks, forced HALF and auto.
streamed-dense is NOT reached: plan_launch names it only for launches of 4M samples and more, which no frame of under 1 000 pixels and
4096 samples is; tests/test_gpu_fast.py's full-size frames are where a request can name it.

MEASURED on the CPU (tests/test_fast_reference.py prints them per case; `python -m tests.fast_cases` prints the table): the worst
diff / allowance of the float32 oracle and of the 16 stand-ins, the share of tight pixels, and the pixels each wrong variant puts beyond
the allowance.  The table as measured is at the end of this docstring.
Worst over all cases: the oracle 0.505, the stand-ins 0.505 (0.5 is a sample that flipped in one run of the ensemble and in the frame: diff = spread).
    case                  spp x bounces  oracle  stand-ins  tight  tight of bouncing  wrong (a)  wrong (b)  of pixels
    1+0_pinhole            23 x 5          0.008   0.251      0.98   0.82                 68        746       851
    1+0_eye                23 x 5          0.007   0.024      0.98   0.84                 67        741       851
    2+0_pinhole            25 x 6          0.009   0.027      0.99   0.99                350        790       851
    2+0_eye                25 x 6          0.008   0.022      1.00   0.99                334        795       851
    3+0_pinhole            12 x 4          0.009   0.500      0.98   0.95                121        805       851
    3+0_eye                12 x 4          0.008   0.248      0.98   0.94                122        795       851
    4+0_pinhole            23 x 5          0.010   0.349      0.92   0.86                312        740       851
    4+0_eye                23 x 5          0.008   0.250      0.93   0.89                340        740       851
    5+0_pinhole            25 x 6          0.009   0.495      0.98   0.96                269        781       851
    5+0_eye                25 x 6          0.010   0.500      0.98   0.96                279        780       851
    6+0_pinhole            12 x 4          0.009   0.249      0.88   0.78                 62        734       851
    6+0_eye                12 x 4          0.008   0.500      0.88   0.79                 53        735       851
    7+0_pinhole            23 x 5          0.009   0.021      0.98   0.97                289        771       851
    7+0_eye                23 x 5          0.010   0.500      0.99   0.98                249        781       851
    8+0_pinhole            25 x 6          0.008   0.500      0.84   0.80                240        710       851
    8+0_eye                25 x 6          0.009   0.250      0.84   0.79                216        717       851
    1+1_pinhole            25 x 4          0.008   0.026      0.98   0.98                602        799       851
    1+1_eye                25 x 4          0.009   0.035      0.97   0.96                550        779       851
    2+1_pinhole            12 x 5          0.009   0.250      0.95   0.94                593        789       851
    2+1_eye                12 x 5          0.007   0.500      0.95   0.93                529        800       851
    3+1_pinhole            23 x 6          0.012   0.441      0.88   0.86                526        728       851
    3+1_eye                23 x 6          0.010   0.500      0.89   0.85                456        717       851
    4+1_pinhole            25 x 4          0.011   0.500      0.88   0.86                454        716       851
    4+1_eye                25 x 4          0.010   0.250      0.90   0.87                414        727       851
    5+1_pinhole            12 x 5          0.009   0.349      0.81   0.79                493        700       851
    5+1_eye                12 x 5          0.009   0.500      0.81   0.76                417        690       851
    6+1_pinhole            23 x 6          0.009   0.036      0.92   0.91                630        766       851
    6+1_eye                23 x 6          0.008   0.251      0.93   0.91                550        781       851
    7+1_pinhole            25 x 4          0.008   0.500      0.81   0.79                501        671       851
    7+1_eye                25 x 4          0.011   0.500      0.82   0.78                439        690       851
    1+2_pinhole            12 x 6          0.009   0.020      0.94   0.94                800        805       851
    1+2_eye                12 x 6          0.009   0.015      0.94   0.94                789        804       851
    2+2_pinhole            23 x 4          0.009   0.014      0.92   0.92                704        769       851
    2+2_eye                23 x 4          0.008   0.020      0.92   0.92                706        774       851
    3+2_pinhole            25 x 5          0.118   0.500      0.82   0.82                502        705       851
    3+2_eye                25 x 5          0.009   0.500      0.79   0.79                424        692       851
    4+2_pinhole            12 x 6          0.013   0.295      0.86   0.86                570        754       851
    4+2_eye                12 x 6          0.013   0.036      0.87   0.87                542        758       851
    5+2_pinhole            23 x 4          0.251   0.500      0.72   0.72                198        587       851
    5+2_eye                23 x 4          0.171   0.500      0.74   0.74                159        603       851
    6+2_pinhole            25 x 5          0.007   0.046      0.94   0.94                488        785       851
    6+2_eye                25 x 5          0.008   0.190      0.94   0.94                400        774       851
    1+3_pinhole            23 x 5          0.010   0.417      0.89   0.89                713        764       851
    1+3_eye                23 x 5          0.008   0.475      0.90   0.90                726        776       851
    2+3_pinhole            25 x 6          0.007   0.500      0.86   0.86                524        749       851
    2+3_eye                25 x 6          0.500   0.500      0.88   0.88                504        755       851
    3+3_pinhole            12 x 4          0.010   0.159      0.89   0.89                557        752       851
    3+3_eye                12 x 4          0.009   0.110      0.88   0.88                482        747       851
    4+3_pinhole            23 x 5          0.053   0.500      0.72   0.72                454        630       851
    4+3_eye                23 x 5          0.157   0.500      0.74   0.74                480        644       851
    5+3_pinhole            25 x 6          0.248   0.500      0.60   0.60                200        509       851
    5+3_eye                25 x 6          0.090   0.500      0.62   0.62                179        540       851
    chunks_17              17 x 4          0.011   0.021      0.89   0.88                 53         79       91
    chunks_33              33 x 4          0.015   0.019      0.82   0.80                 53         75       91
    chunks_71              71 x 4          0.013   0.016      0.82   0.80                 53         74       91
    chunks_144            144 x 4          0.016   0.011      0.76   0.73                 51         64       91
    chunks_250            250 x 4          0.018   0.046      0.76   0.73                 51         57       91
    chunks_272            272 x 4          0.015   0.205      0.76   0.73                 51         49       91
    chunks_520            520 x 4          0.019   0.250      0.69   0.66                 49         42       91
    field24_pinhole        23 x 4          0.010   0.500      0.62   0.61                262        543       851
    field24_orthographic   23 x 4          0.012   0.500      0.56   0.56                164        526       851
    field45_scalar_load    12 x 4          0.505   0.505      0.63   0.63                376        621       851"""
import dataclasses
import functools
import zlib

import numpy as np

import rt_amd
from oracle import binding as oracle
from rt_amd import capi
from tests import fast_reference as ref
from tests import lds_plan

A, R, S = 64.0, 32, 4.0
STAND_INS = 16  # half at S, half at S / 2

FAST = capi.RT_HIP_FLAG_FAST
WHOLE = capi.RT_HIP_FLAG_FORCE_WHOLE_CHUNKS
HALF = capi.RT_HIP_FLAG_FORCE_HALF_CHUNKS
RESIDENT = capi.RT_HIP_FLAG_FORCE_RESIDENT
TILED = capi.RT_HIP_FLAG_FORCE_TILED
STREAMED = capi.RT_HIP_FLAG_FORCE_STREAMED
DEVICE_LDS = 160 * 1024  # (tests/test_gpu_chunk_sweep.py: what the MI355X gives a workgroup)
SCAN_TILED, SCAN_STREAMED, SCAN_STREAMED_DENSE = -1, -2, -3
CAMERA_FORMS = {"pinhole": 0, "eye": 1, "general": 2}
MAX_BOUNCES = 6
CHANNEL_RATIO = 0.5 ** (MAX_BOUNCES + 1)


@dataclasses.dataclass(frozen=True)
class Variant:
    label: str
    flags: int  # beside RT_HIP_FLAG_FAST
    kernel: str  # what stats["kernel"] must say
    scan: int
    planes: int
    general_camera: int
    halves: int
    chunks: int
    pixels_log2: int


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    sweep: str  # "builds", "chunks" or "kernels"
    scene: tuple  # (spheres, planes, camera): what pod_of builds from
    width: int
    height: int
    spp: int
    bounces: int
    seed: int
    variants: tuple
    hbm: bool = False  # also through rt_hip_render_device into a tensor
    stripes: bool = False  # also as partition = (rank, 3, 5)


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------
PINHOLE = ((0.0, 1.0, 3.0), (0.0, -0.2, -1.0))
TILTED = ((0.2, 1.2, 3.0), (0.0, -0.15, -1.0))  # (tests/test_gpu_parity.py: rounding noise in the last row's x / y terms: the eye form)
# clip -> world: parallel rays looking down at the floor, no finite eye; the near plane close in front of the scene (e.e - (e.d)^2 cancels:
# what rounding does to a hit grows with the distance the ray has come, and with it the spread)
ORTHOGRAPHIC = ((3.2, 0, 0, 0.1), (0, 1.4, -6.0, 1.9), (0, 0, -10, 1.0), (0, 0, 0, 1))


def materials_of(rng, n=4):
    """(type, r, g, b, a, roughness, reflectivity): lambert (0) or metal (1), albedo channels in [0.5, 1], albedo x reflectivity <= 1"""
    return [(int(rng.integers(0, 2)), *rng.uniform(0.5, 1.0, 3), 1.0, rng.uniform(0.0, 0.5), rng.uniform(0.6, 1.0)) for _ in range(n)]


def planes_of(rng, n):
    """a floor below the camera, then a back wall, then a wall on the left: each slightly off its axis"""
    planes = [(0.0, 1.0, 0.0, rng.uniform(0.0, 0.5), rng.integers(0, 4)), (0.1, 0.05, 1.0, 8.0, rng.integers(0, 4)), (1.0, 0.05, 0.1, 5.0, rng.integers(0, 4))][:n]
    return [(*(np.array(p[:3]) / np.linalg.norm(p[:3])), p[3], p[4]) for p in planes]


@functools.lru_cache(maxsize=None)
def geometry(n_spheres, n_planes):
    rng = np.random.default_rng(7000 + 16 * n_planes + n_spheres)
    materials = materials_of(rng)
    if n_spheres <= 8 and n_planes == 0:  # nothing but spheres and sky: large ones close to the camera, which fill the frame
        spheres = [(rng.uniform(-2.5, 2.5), rng.uniform(0.0, 2.0), rng.uniform(-2.5, 0.0), rng.uniform(0.9, 1.4), rng.integers(0, 4)) for _ in range(n_spheres)]
    elif n_spheres <= 8:
        spheres = [(rng.uniform(-2.5, 2.5), rng.uniform(0.2, 1.8), rng.uniform(-5.0, -1.0), rng.uniform(0.5, 1.1), rng.integers(0, 4)) for _ in range(n_spheres)]
    else:  # a few dozen: rows of small ones standing on the floor's height
        columns = 6
        spheres = [(-3.1 + 1.25 * (i % columns) + rng.uniform(-0.1, 0.1), 0.5 + 0.9 * ((i // columns) % 2), -0.5 - 1.2 * (i // columns) + rng.uniform(-0.1, 0.1), rng.uniform(0.45, 0.6), rng.integers(0, 4)) for i in range(n_spheres)]
    return spheres, planes_of(rng, n_planes), materials


@functools.lru_cache(maxsize=None)
def matrix_of(camera, width, height):
    if camera == "orthographic":
        return tuple(float(np.float32(v)) for row in ORTHOGRAPHIC for v in row)
    return tuple(rt_amd.Scene.parse("").set_camera(*{"pinhole": PINHOLE, "eye": TILTED}[camera]).describe(width, height).inverse_view_projection[:])


def pod_of(case):
    n_spheres, n_planes, camera = case.scene
    spheres, planes, materials = geometry(n_spheres, n_planes)
    return rt_amd.scene_from_arrays(spheres, planes, materials, samples_per_pixel=case.spp, max_bounces=case.bounces, inverse_view_projection=list(matrix_of(camera, case.width, case.height)))


# ---- the table -------------------------------------------------------------------------------------------------------------------------
PAIRS = [(s, p) for p in range(4) for s in range(1, 9 - p)]  # the 26 builds of the scalar-register kernel
HBM_PAIRS = {(1, 0), (8, 0), (3, 1), (7, 1), (4, 2), (5, 3)}
STRIPE_PAIRS = {(2, 0), (6, 1), (3, 3)}
BUILD_SAMPLES = (12, 23, 25)
# K: (pixels_log2 in whole chunks, in HALF) at 37 x 23 (choose_queue: 128 items per wave, 64 for a frame this small; HALF 64 half-chunks)
BUILD_TILES = {1: (6, 5), 2: (5, 4)}
# 13 x 7 — spp: (K, pixels_log2 auto, pixels_log2 in whole chunks, HALF under auto)
CHUNK_SAMPLES = {17: (2, 4, 5, 1), 33: (3, 3, 4, 1), 71: (5, 2, 3, 1), 144: (9, 2, 2, 1), 250: (16, 2, 2, 1), 272: (17, 2, 2, 0), 520: (33, 2, 2, 0)}
CHUNK_PAIR = (3, 1)


def build_cases():
    out = []
    for s, p in PAIRS:
        for camera in ("pinhole", "eye"):
            spp = BUILD_SAMPLES[(s + p) % 3]
            chunks = -(-spp // 16)
            whole, half = BUILD_TILES[chunks]
            variants = (Variant("whole", WHOLE, "small", s, p, int(camera == "eye"), 0, chunks, whole), Variant("half", HALF, "small", s, p, int(camera == "eye"), 1, chunks, half))
            out.append(Case(f"{s}+{p}_{camera}", "builds", (s, p, camera), 37, 23, spp, 4 + (s + 2 * p) % 3, 100 * s + 10 * p + (camera == "eye"), variants, hbm=(s, p) in HBM_PAIRS, stripes=(s, p) in STRIPE_PAIRS and camera == "pinhole"))
    return out


def chunk_cases():
    out = []
    s, p = CHUNK_PAIR
    for spp, (chunks, log2_auto, log2_whole, half) in CHUNK_SAMPLES.items():
        variants = []
        for kernel, flags, scan, planes in (("small", 0, s, p), ("resident", RESIDENT, 0, 0)):
            variants.append(Variant(f"{kernel}_whole", flags | WHOLE, kernel, scan, planes, 0, 0, chunks, log2_whole))
            variants.append(Variant(f"{kernel}_auto", flags, kernel, scan, planes, 0, half, chunks, log2_auto))
        out.append(Case(f"chunks_{spp}", "chunks", (s, p, "pinhole"), 13, 7, spp, 4, 500 + spp, tuple(variants), hbm=spp in (33, 272)))
    return out


def kernel_cases():
    def forms(kernel, flags, scan, planes, general):
        """whole chunks, forced HALF and auto at 23 samples (K = 2): a tile-per-wave launch this small takes HALF by itself; the rolling
        kernels halve their items only when forced (their auto rule asks for 1025 primitives)"""
        big = scan < 0
        return (Variant(f"{kernel}_whole", flags | WHOLE, kernel, scan, planes, general, 0, 2, 0 if big else 5), Variant(f"{kernel}_half", flags | HALF, kernel, scan, planes, general, 1, 2, 0 if big else 4),
                Variant(f"{kernel}_auto", flags, kernel, scan, planes, general, 0 if big else 1, 2, 0 if big else 4))

    return [
        Case("field24_pinhole", "kernels", (24, 1, "pinhole"), 37, 23, 23, 4, 901, forms("resident", RESIDENT, 0, 0, 0) + forms("tiled", TILED, SCAN_TILED, 0, 0) + forms("streamed", STREAMED, SCAN_STREAMED, 0, 0), hbm=True, stripes=True),
        Case("field24_orthographic", "kernels", (24, 1, "orthographic"), 37, 23, 23, 4, 902, forms("resident", RESIDENT, 0, 0, 1), hbm=True),
        Case("field45_scalar_load", "kernels", (45, 1, "pinhole"), 37, 23, 12, 4, 903, (Variant("resident_whole", RESIDENT | WHOLE, "resident", 0, 1, 0, 0, 1, 6), Variant("resident_half", RESIDENT | HALF, "resident", 0, 1, 0, 1, 1, 5),
                                                                                   Variant("resident_auto", RESIDENT, "resident", 0, 1, 0, 0, 1, 6))),
    ]


CASES = build_cases() + chunk_cases() + kernel_cases()
BY_NAME = {case.name: case for case in CASES}
assert len(BY_NAME) == len(CASES)


def of_sweep(sweep):
    return [case for case in CASES if case.sweep == sweep]


# ---- what every case shares: computed once, read-only -----------------------------------------------------------------------------------
def noise_seed(case, checks=False):
    """ensemble seeds are even, the stand-ins' odd: disjoint"""
    return 2 * zlib.crc32(case.name.encode()) + int(checks)


@functools.lru_cache(maxsize=None)
def reference(name):
    """the per-pixel rule of the case's frame (fast_reference.Allowance)"""
    case = BY_NAME[name]
    return ref.allowance_of(pod_of(case), case.width, case.height, case.seed, A, R, noise_seed(case))


@functools.lru_cache(maxsize=None)
def oracle_frame(name):
    """the float32 oracle's frame: (rgba, float mean, segments)"""
    case = BY_NAME[name]
    rgba, rgb, stats = oracle.render(pod_of(case), case.width, case.height, seed=case.seed)
    rgba.setflags(write=False), rgb.setflags(write=False)
    return rgba, rgb, stats["segments"]


@functools.lru_cache(maxsize=None)
def check_frames(name):
    """(stand-ins [STAND_INS, h, w, 3]: single runs at S and S / 2 ulps; wrong variant (a): the unit vector scaled by 1.001; wrong variant
    (b): each pixel's last sample from the next sample index's stream)"""
    case = BY_NAME[name]
    runs = [ref.Run(amplitude=S)] * (STAND_INS // 2) + [ref.Run(amplitude=S / 2)] * (STAND_INS // 2) + [ref.Run(unit_scale=1.001), ref.Run(shift_last=True)]
    frames, _ = ref.trace(pod_of(case), case.width, case.height, case.seed, runs=runs, noise_seed=noise_seed(case, checks=True))
    frames.setflags(write=False)
    return frames[:STAND_INS], frames[STAND_INS], frames[STAND_INS + 1]


def camera_of(case, pod=None):
    return CAMERA_FORMS[oracle.primary_ray(pod if pod is not None else pod_of(case), case.width, case.height, 0, 0, want_form=True)[2]]


def planned(case, variant, host, rows=None):
    """plan_launch as render.hip asks it for the case's frame (or `rows` local rows of it) under FAST and the variant's flags"""
    n_spheres, n_planes, _ = case.scene
    return lds_plan.plan(n_spheres, n_planes, case.width, case.height if rows is None else rows, case.spp, camera=camera_of(case), flags=FAST | variant.flags, host_frame=host, lds_limit=DEVICE_LDS)


def assert_plan(case, variant, host, rows=None):
    """the frame takes the build the table names: a later change of launch policy cannot silently empty a case"""
    p = planned(case, variant, host, rows)
    got = (p["scan"], p["planes"], p["general_camera"], p["sub_chunk_items"], p["halves"], p["chunks"], p["pixels_log2"], p["refusal"])
    want = (variant.scan, variant.planes, variant.general_camera, variant.halves, variant.halves, variant.chunks, variant.pixels_log2, "")
    assert got == want, (case.name, variant.label, host, rows, got, want)
    return p


def instantiation(variant):
    """the fast instantiation of render_queue a variant's plan names, as DESIGN.md counts them"""
    items = "HALF" if variant.halves else "whole"
    if variant.scan > 0:
        return f"scalar-register ({variant.scan} spheres, {variant.planes} planes), {'eye' if variant.general_camera else 'pinhole'}, {items}"
    if variant.scan == 0:
        return f"resident ({'scalar-load scan' if variant.planes else 'LDS scan, general camera' if variant.general_camera else 'LDS scan, pinhole'}), {items}"
    return f"{ {SCAN_TILED: 'tiled', SCAN_STREAMED: 'streamed', SCAN_STREAMED_DENSE: 'streamed-dense'}[variant.scan]}, {items}"


def stripe_rows(height, rank, world=3, stripe=5):
    return [y for y in range(height) if (y // stripe) % world == rank]


if __name__ == "__main__":
    print("case: spp x bounces | oracle worst diff/allowance | stand-ins worst | tight share | wrong (a), (b) pixels beyond")
    for case in CASES:
        rule = reference(case.name)
        stand_ins, wrong_a, wrong_b = check_frames(case.name)
        print(f"{case.name}: {case.spp} x {case.bounces} | {rule.excess(oracle_frame(case.name)[1]).max():.3f} | {max(rule.excess(f).max() for f in stand_ins):.3f} | {rule.tight.mean():.2f} (of bouncing pixels {rule.tight[rule.bounced].mean():.2f}) | "
              f"{int((rule.excess(wrong_a) > 1).sum())}, {int((rule.excess(wrong_b) > 1).sum())}", flush=True)
