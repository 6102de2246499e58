"""What a render launch is told before it is planned (rt_amd/csrc/frame_setup.cpp), on the CPU: the refusals of rt_hip_render_device
(check_render_request) and the per-frame constants every pixel is traced from (make_frame_params, camera_form_of).

tests/native/frame_setup_dump.cpp and frame_setup.cpp are built with g++ alone — nothing of ROCm on the command line, which is the
proof that the unit is host-only — and every field of frame_params is compared BIT FOR BIT with the oracle's independent copy of the
arithmetic (oracle/cpu_ref.cpp make_frame, through oracle_frame_constants).  The messages and statuses of the refusals were recorded
when the lines had only been moved out of render.hip.

One case the camera's classification names cannot be made: a finite matrix that fails ONLY the pinhole's "near point's motion is
kappa times the near-to-far vector's, to 1e-5" test.  With a w row free of x and y the near and far points share the matrix's x and y
columns, so o1 = mx sx / w_near and d1 = mx sx (1 / w_far - 1 / w_near) are proportional by construction, with the same
kappa = (1 / w_near) / (1 / w_far - 1 / w_near) in every component; what binary64's roundings leave of o1 - kappa d1 is about
2^-53 (kappa + 1) of the scale, at most 2^-32 because kappa is held below 2^20 — never 1e-5.  A frustum sheared in x and y alone is therefore still a pinhole's
(an off-axis one: the test below says so and holds its constants against the oracle's); a matrix leaves the pinhole form through its
w row, its kappa, or a near-to-far vector that does not move with the pixel (the orthographic one)."""
import shutil
import struct
import subprocess

import numpy as np
import pytest

import rt_amd
from oracle import binding as oracle
from rt_amd import capi
from tests.conftest import ROOT

SOURCES = [str(ROOT / "tests" / "native" / "frame_setup_dump.cpp"), str(ROOT / "rt_amd" / "csrc" / "frame_setup.cpp")]
SIZES = [(1, 1), (96, 54), (1920, 1080), (3, 65535)]
SEEDS = [0, 1, (1 << 32) + 7, (1 << 64) - 1]
PINHOLE, PLAIN_EYE, OTHER = 0, 1, 2  # camera_form
OK, INVALID_ARGUMENT, UNSUPPORTED = 0, 1, 5  # rt_hip_status
RAY_FIELDS = ["ray_d0", "ray_d1", "ray_d2", "ray_j1", "ray_j2", "ray_eye"]
EYE_FIELDS = ["eye_q0", "eye_q1", "eye_q2", "eye_jq1", "eye_jq2", "eye_w0", "eye_w1", "eye_w2", "eye_jw1", "eye_jw2", "eye_e", "eye_zws"]


def bits(x: float) -> int:
    return struct.unpack("<I", struct.pack("<f", x))[0]


def matrix_of(pod):
    return [float(v) for v in pod.inverse_view_projection]


def axis_aligned(width, height):
    return matrix_of(rt_amd.Scene.named("basic").describe(width, height))


def tilted(width, height):  # (tests/test_oracle_kat.py, test_primary_ray_for_rotated_camera)
    return matrix_of(rt_amd.Scene.named("basic").set_camera((1.0, 2.0, 3.0), (0.3, -0.2, -1.0)).describe(width, height))


def noisy_w_row(width, height):  # (tests/test_oracle_kat.py: "x matters" to w by one part in 10^12)
    m = axis_aligned(width, height)
    m[12] = 1.0e-12 * m[15]
    return m


def orthographic(width, height):  # (tests/test_oracle_kat.py)
    return [2.0, 0, 0, 0, 0, 1.25, 0, 1.0, 0, 0, -10.0, 3.0, 0, 0, 0, 1.0]


def sheared(width, height):  # x leans on y and y on x: an off-axis frustum, every near-to-far line still through one point
    m = axis_aligned(width, height)
    m[1], m[4] = 0.3 * m[0], -0.2 * m[5]
    return m


CAMERAS = {"axis_aligned": axis_aligned, "tilted": tilted, "noisy_w_row": noisy_w_row, "orthographic": orthographic, "sheared": sheared}
HAS_EYE = {"axis_aligned", "tilted", "noisy_w_row", "sheared"}


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("frame_setup") / "frame_setup_dump"
    # (no include path but the sources' own relative ones: no HIP header can be found)
    built = subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", *SOURCES, "-o", str(exe)], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr

    def run(lines):
        out = subprocess.run([str(exe)], input="".join(line + "\n" for line in lines), capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr
        got = out.stdout.splitlines()
        assert len(got) == len(lines)
        return got

    return run


def frame_line(matrix, width, height, rank=0, world=1, stripe_rows=8, samples=64, bounces=8, seed=0, whole=0):
    words = " ".join(f"{bits(v):x}" for v in matrix)
    return f"frame {width} {height} {rank} {world} {stripe_rows} {samples} {bounces} {seed} {whole} {words}"


def parse_frame(line):
    kind, *fields = line.split()
    assert kind == "frame"
    return {name: tuple(int(w, 16) for w in value.split(",")) for name, value in (f.split("=") for f in fields)}


def frames(dump, requests):
    """requests: keyword arguments of frame_line -> the parsed frame_params, scalars unwrapped"""
    return [{k: (v[0] if len(v) == 1 else v) for k, v in parse_frame(line).items()} for line in dump([frame_line(**r) for r in requests])]


def oracle_constants(matrix, width, height, seed):
    pod = rt_amd.Scene.named("basic").describe(width, height)
    for i, v in enumerate(matrix):
        pod.inverse_view_projection[i] = v
    return {k: (v[0] if len(v) == 1 else v) for k, v in oracle.frame_constants(pod, width, height, seed).items()}


def test_every_constant_has_the_oracles_bits(dump):
    cases = [(name, size, seed) for name in CAMERAS for size in SIZES for seed in SEEDS]
    got = frames(dump, [dict(matrix=CAMERAS[name](*size), width=size[0], height=size[1], seed=seed) for name, size, seed in cases])
    for (name, (width, height), seed), f in zip(cases, got):
        where = (name, width, height, seed)
        want = oracle_constants(CAMERAS[name](width, height), width, height, seed)
        assert (f["pinhole"] != 0) == (want["pinhole_rays"] != 0), where
        assert (f["eye_form"] != 0) == (want["eye_rays"] != 0), where
        for field in RAY_FIELDS + EYE_FIELDS + ["mx", "my", "k_near", "k_far", "sx", "frame_key_a", "frame_key_b"]:
            assert f[field] == want[field], (where, field, f[field], want[field])
        # a form that does not apply: its scalars are left as they were initialised, on both sides
        if not f["pinhole"]:
            assert all(f[field] == (0, 0, 0) for field in RAY_FIELDS) and all(want[field] == (0, 0, 0) for field in RAY_FIELDS), where
        if not f["eye_form"]:
            assert all(f[field] in (0, (0, 0, 0)) for field in EYE_FIELDS) and all(want[field] in (0, (0, 0, 0)) for field in EYE_FIELDS), where
        assert f["neg_sy"] == bits(-float(np.float32(2.0) / np.float32(height))), where
        assert (f["width"], f["height"]) == (width, height), where


def test_the_key_halves_change_with_either_half_of_the_seed(dump):
    got = frames(dump, [dict(matrix=axis_aligned(96, 54), width=96, height=54, seed=seed) for seed in SEEDS])
    assert len({(f["frame_key_a"], f["frame_key_b"]) for f in got}) == len(SEEDS)


def test_classification_of_the_cameras(dump):
    cases = [(name, size) for name in CAMERAS for size in SIZES]
    got = frames(dump, [dict(matrix=CAMERAS[name](*size), width=size[0], height=size[1]) for name, size in cases])
    for (name, size), f in zip(cases, got):
        # every camera with an eye is a plain one: no reciprocal guard, no flip
        assert f["eye_form"] == (2 if name in HAS_EYE else 0), (name, size)
        pinhole = name in ("axis_aligned", "sheared")  # (sheared: see the module's docstring)
        assert f["pinhole"] == (1 if pinhole else 0), (name, size)
        assert f["camera_form"] == (PINHOLE if pinhole else PLAIN_EYE if name in HAS_EYE else OTHER), (name, size)


def test_classification_at_its_edges(dump):
    width, height = 96, 54
    base = axis_aligned(width, height)
    k_near_w = base[15]  # fma(M[14], 0, M[15])
    assert base[12] == 0.0 and base[13] == 0.0 and base[14] != 0.0 and k_near_w != 0.0

    def with_(**changes):
        m = list(base)
        for index, value in changes.items():
            m[int(index[1:])] = value
        return m

    # rt's camera: near w = M15 = 1 / near, far w = M14 + M15 = 1 / far, both positive, the far one 10^5 times the smaller.  A w row that
    # leans on x or y by `lean` moves BOTH by -+lean across the frame: a thousandth of the far w leaves every sign alone
    w_far = base[14] + base[15]
    assert k_near_w > 0.0 and 0.0 < w_far < 1.0e-3 * k_near_w
    lean = 1.0e-3 * w_far

    def scaled(factor, lean=0.0):  # the w row alone: w at every corner is `factor` times what it is with a lean of `lean`
        m = list(base)
        m[12], m[14], m[15] = lean * factor, base[14] * factor, base[15] * factor
        return m

    named = {
        # near-plane w = k + M12 (X - ... ) runs from k - M12 at the left edge to k + M12 at the right one
        "w_changes_sign": with_(m12=2.0 * k_near_w),
        "w_zero_at_a_corner": with_(m12=k_near_w),
        "w_above_the_band": scaled(2.0**52 / k_near_w, lean),
        "w_below_the_band": scaled(2.0**-52 / k_near_w, lean),
        "pinhole_w_above_the_band": scaled(2.0**52 / k_near_w),
        "no_depth_in_w": with_(m14=0.0),
        "nan_in_depth_column": with_(m6=float("nan")),
        "inf_in_depth_column": with_(m2=float("inf")),
        "w_leans_on_x": with_(m12=lean),
        "w_leans_on_y": with_(m13=lean),
        "far_w_changes_sign": with_(m12=100.0 * w_far),
        # kappa = w_far / (w_near - w_far) = (M14 + M15) / -M14: the depth term of w decides it
        "kappa_too_large": with_(m14=-base[15] * 2.0**-22),  # 2^22 - 1: near and far w almost equal
        "kappa_too_small": with_(m14=base[15] * (2.0**-22 - 1.0)),  # 2^-22 and a bit: the far w 2^-22 of the near one
        "kappa_negative": with_(m14=-3.0 * base[15]),  # -2/3: the far w on the other side of zero
    }
    got = dict(zip(named, frames(dump, [dict(matrix=m, width=width, height=height) for m in named.values()])))
    forms = {name: (f["pinhole"], f["eye_form"], f["camera_form"]) for name, f in got.items()}
    assert forms["w_changes_sign"] == (0, 1, OTHER)
    assert forms["w_zero_at_a_corner"] == (0, 1, OTHER)
    assert forms["w_above_the_band"] == (0, 1, OTHER) and forms["w_below_the_band"] == (0, 1, OTHER)
    assert forms["pinhole_w_above_the_band"] == (1, 1, PINHOLE)  # (kappa does not change with w's scale: the pinhole form outranks the eye form)
    assert forms["no_depth_in_w"][1] == 0 and forms["nan_in_depth_column"][1] == 0 and forms["inf_in_depth_column"][1] == 0
    assert forms["w_leans_on_x"] == (0, 2, PLAIN_EYE) and forms["w_leans_on_y"] == (0, 2, PLAIN_EYE)
    assert forms["far_w_changes_sign"] == (0, 1, OTHER)  # (the near w keeps its sign: it is the far one that crosses zero)
    for name in ("kappa_too_large", "kappa_too_small", "kappa_negative"):
        assert forms[name][0] == 0, name
    assert forms["kappa_too_large"][1:] == (2, PLAIN_EYE) and forms["kappa_too_small"][1:] == (2, PLAIN_EYE)
    assert forms["kappa_negative"][1:] == (1, OTHER)  # near and far on opposite sides of w = 0: the flip is needed
    # a frame without an eye and without a pinhole goes through the homogeneous form
    assert forms["no_depth_in_w"] == (0, 0, OTHER)
    # ... and all of it is what the oracle decides, bit for bit
    for name, matrix in named.items():
        want = oracle_constants(matrix, width, height, 0)
        f = got[name]
        assert ((f["pinhole"] != 0), (f["eye_form"] != 0)) == ((want["pinhole_rays"] != 0), (want["eye_rays"] != 0)), name
        for field in RAY_FIELDS + EYE_FIELDS + ["mx", "my", "k_near", "k_far"]:
            assert f[field] == want[field], (name, field)


def local_rows(height, rank, world, stripe_rows):
    """rt_hip_partition's rule (include/rt_hip.h): stripes of stripe_rows rows, dealt to the ranks in turn; the last one may be short"""
    stripes = -(-height // stripe_rows)
    return sum(min(stripe_rows, height - b * stripe_rows) for b in range(rank, stripes, world))


def test_the_plain_fields(dump):
    m = axis_aligned(96, 54)
    for stripe_rows, shift in [(1, 0), (8, 3), (256, 8), (6, 0xFFFFFFFF)]:
        (f,) = frames(dump, [dict(matrix=m, width=96, height=54, stripe_rows=stripe_rows)])
        assert f["stripe_shift"] == shift and f["stripe_rows"] == stripe_rows
    cases = [(height, rank, world, stripe_rows) for height in (1, 54, 1080) for rank, world in ((0, 1), (0, 8), (7, 8)) for stripe_rows in (8, 6)]
    got = frames(dump, [dict(matrix=m, width=96, height=h, rank=r, world=w, stripe_rows=s) for h, r, w, s in cases])
    for (height, rank, world, stripe_rows), f in zip(cases, got):
        assert f["local_rows"] == local_rows(height, rank, world, stripe_rows), (height, rank, world, stripe_rows)
        assert (f["rank"], f["world"], f["height"]) == (rank, world, height)
    # the padded height is the largest share, and the shares add up to the frame
    for height in (1, 54, 1080):
        shares = [local_rows(height, r, 8, 8) for r in range(8)]
        assert sum(shares) == height and max(shares) == local_rows(height, 0, 8, 8)
    for bounces, want in [(0, 0), (8, 8), (1 << 30, 1 << 30), ((1 << 30) + 1, 1 << 30), (0xFFFFFFFF, 1 << 30)]:
        (f,) = frames(dump, [dict(matrix=m, width=96, height=54, bounces=bounces)])
        assert f["max_bounces"] == want
    for samples in (1, 64, 4096):
        (f,) = frames(dump, [dict(matrix=m, width=96, height=54, samples=samples)])
        assert f["samples_per_pixel"] == samples
    assert [f["frame_rows"] for f in frames(dump, [dict(matrix=m, width=96, height=54, whole=w) for w in (0, 1)])] == [0, 1]


F = capi
REFUSALS = [
    # (width, height, flags, partition or None) -> status, message: one row per refusal, texts as render.hip gave them
    ((0, 54, 0, None), INVALID_ARGUMENT, "rt_hip_render_device: empty frame 0x54"),
    ((96, 0, 0, None), INVALID_ARGUMENT, "rt_hip_render_device: empty frame 96x0"),
    ((65536, 65536, 0, None), INVALID_ARGUMENT, "rt_hip_render_device: 65536x65536 exceeds the 32-bit pixel index of image_view"),
    ((96, 54, 1 << 12, None), UNSUPPORTED, "rt_hip_render_device: unknown flag bits 0x1000"),
    ((96, 54, (1 << 31) | F.RT_HIP_FLAG_FAST, None), UNSUPPORTED, "rt_hip_render_device: unknown flag bits 0x80000040"),
    ((96, 54, F.RT_HIP_FLAG_BVH | F.RT_HIP_FLAG_FORCE_TILED, None), UNSUPPORTED, "rt_hip_render_device: RT_HIP_FLAG_BVH chooses its own kernel (not with RT_HIP_FLAG_FORCE_TILED / _RESIDENT / _STREAMED)"),
    ((96, 54, F.RT_HIP_FLAG_BVH | F.RT_HIP_FLAG_FORCE_RESIDENT, None), UNSUPPORTED, "rt_hip_render_device: RT_HIP_FLAG_BVH chooses its own kernel (not with RT_HIP_FLAG_FORCE_TILED / _RESIDENT / _STREAMED)"),
    ((96, 54, F.RT_HIP_FLAG_BVH | F.RT_HIP_FLAG_FORCE_STREAMED, None), UNSUPPORTED, "rt_hip_render_device: RT_HIP_FLAG_BVH chooses its own kernel (not with RT_HIP_FLAG_FORCE_TILED / _RESIDENT / _STREAMED)"),
    ((96, 54, F.RT_HIP_FLAG_BVH | F.RT_HIP_FLAG_FAST, None), UNSUPPORTED, "rt_hip_render_device: RT_HIP_FLAG_BVH is built for the parity contract's arithmetic only (not with RT_HIP_FLAG_FAST)"),
    # (with the preview the BVH bits are dropped BEFORE this check, after the two above: PREVIEW + BVH + FAST is refused for BVH + FAST)
    ((96, 54, F.RT_HIP_FLAG_PREVIEW | F.RT_HIP_FLAG_BVH | F.RT_HIP_FLAG_FAST, None), UNSUPPORTED, "rt_hip_render_device: RT_HIP_FLAG_BVH is built for the parity contract's arithmetic only (not with RT_HIP_FLAG_FAST)"),
    ((96, 54, F.RT_HIP_FLAG_BVH_DEVICE_BUILD, None), UNSUPPORTED, "rt_hip_render_device: RT_HIP_FLAG_BVH_DEVICE_BUILD says how RT_HIP_FLAG_BVH's hierarchy is built (not without it)"),
    ((96, 54, F.RT_HIP_FLAG_FORCE_HALF_CHUNKS | F.RT_HIP_FLAG_FORCE_WHOLE_CHUNKS, None), INVALID_ARGUMENT, "rt_hip_render_device: RT_HIP_FLAG_FORCE_HALF_CHUNKS and RT_HIP_FLAG_FORCE_WHOLE_CHUNKS exclude each other"),
    ((96, 54, F.RT_HIP_FLAG_FAST | F.RT_HIP_FLAG_SM_MATERIALS, None), UNSUPPORTED, "rt_hip_render_device: RT_HIP_FLAG_FAST applies to mg_ray_tracer's path only (not with RT_HIP_FLAG_SM_MATERIALS / RT_HIP_FLAG_PREVIEW)"),
    ((96, 54, F.RT_HIP_FLAG_FAST | F.RT_HIP_FLAG_PREVIEW, None), UNSUPPORTED, "rt_hip_render_device: RT_HIP_FLAG_FAST applies to mg_ray_tracer's path only (not with RT_HIP_FLAG_SM_MATERIALS / RT_HIP_FLAG_PREVIEW)"),
    ((3, 131071, 0, None), INVALID_ARGUMENT, "rt_hip_render_device: frame height 131071 exceeds the supported 131070 rows"),
    ((96, 54, 0, (0, 0, 8)), INVALID_ARGUMENT, "rt_hip_render_device: invalid partition {rank 0, world 0, stripe_rows 8}"),
    ((96, 54, 0, (8, 8, 8)), INVALID_ARGUMENT, "rt_hip_render_device: invalid partition {rank 8, world 8, stripe_rows 8}"),
    ((96, 54, 0, (1, 3, 0)), INVALID_ARGUMENT, "rt_hip_render_device: invalid partition {rank 1, world 3, stripe_rows 0}"),
]
LEGAL_ALONE = [F.RT_HIP_FLAG_FORCE_TILED, F.RT_HIP_FLAG_FORCE_RESIDENT, F.RT_HIP_FLAG_PERSISTENT_FRAME, F.RT_HIP_FLAG_SM_MATERIALS, F.RT_HIP_FLAG_PREVIEW,
               F.RT_HIP_FLAG_FORCE_STREAMED, F.RT_HIP_FLAG_FAST, F.RT_HIP_FLAG_STATS, F.RT_HIP_FLAG_FORCE_HALF_CHUNKS, F.RT_HIP_FLAG_FORCE_WHOLE_CHUNKS, F.RT_HIP_FLAG_BVH]


def check_line(width, height, flags, partition):
    rank, world, stripe_rows = partition or (0, 0, 0)
    return f"check {width} {height} {flags:x} {1 if partition else 0} {rank} {world} {stripe_rows}"


def parse_check(line):
    head, _, message = line.partition(" | ")
    kind, *fields = head.split()
    assert kind == "check"
    values = dict(f.split("=") for f in fields)
    return {"status": int(values["status"]), "flags": int(values["flags"], 16), "bvh_device_build": int(values["bvh_device_build"]),
            "partition": (int(values["rank"]), int(values["world"]), int(values["stripe_rows"])), "message": message}


def test_refusals_keep_their_status_and_text(dump):
    got = [parse_check(line) for line in dump([check_line(*request) for request, _, _ in REFUSALS])]
    for (request, status, message), c in zip(REFUSALS, got):
        assert (c["status"], c["message"]) == (status, message), request


def test_accepted_requests(dump):
    whole = (0, 1, capi.RT_HIP_DEFAULT_STRIPE_ROWS)
    BVH, BUILD, PREVIEW = F.RT_HIP_FLAG_BVH, F.RT_HIP_FLAG_BVH_DEVICE_BUILD, F.RT_HIP_FLAG_PREVIEW
    # request -> the launch's flags, "build the hierarchy on the device", the partition
    rows = [((96, 54, 0, None), 0, 0, whole)]
    rows += [((96, 54, flag, None), flag, 0, whole) for flag in LEGAL_ALONE]
    rows += [((96, 54, BVH | BUILD, None), BVH, 1, whole)]  # the builder's flag does not travel to the launch
    rows += [((96, 54, PREVIEW | BVH, None), PREVIEW, 0, whole), ((96, 54, PREVIEW | BVH | BUILD, None), PREVIEW, 0, whole), ((96, 54, PREVIEW | BUILD, None), PREVIEW, 0, whole)]
    rows += [((96, 54, BVH | F.RT_HIP_FLAG_SM_MATERIALS | F.RT_HIP_FLAG_FORCE_HALF_CHUNKS, (7, 8, 6)), BVH | F.RT_HIP_FLAG_SM_MATERIALS | F.RT_HIP_FLAG_FORCE_HALF_CHUNKS, 0, (7, 8, 6))]
    rows += [((3, 131070, 0, (0, 1, 1)), 0, 0, (0, 1, 1)), ((65535, 65537, 0, None), 0, 0, whole)]  # the largest frames taken: 131070 rows; 2^32 - 1 pixels
    got = [parse_check(line) for line in dump([check_line(*request) for request, *_ in rows])]
    for (request, flags, build, partition), c in zip(rows, got):
        assert c == {"status": OK, "flags": flags, "bvh_device_build": build, "partition": partition, "message": ""}, request
