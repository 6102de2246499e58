"""What the tests of RT_HIP_FLAG_BVH_DEVICE_BUILD share (tests/test_bvh_lbvh_reference.py on the CPU,
tests/test_gpu_bvh_device_build.py and tests/test_gpu_bvh_device_build_scale.py on the GPU): the serial restatement of the device builder (tests/native/lbvh_reference.cpp,
built with g++ alone), the scenes both suites build trees of, and a numpy model of the builder's keys and of its uncapped cut."""
import functools
import shutil
import subprocess
import tempfile
from pathlib import Path

import numpy as np

from tests import bvh_cases

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / "tests" / "native" / "lbvh_reference.cpp"


@functools.lru_cache(maxsize=None)
def reference_binary():
    """tests/native/lbvh_reference.cpp compiled with g++ alone (nothing of ROCm on the command line); None without g++."""
    cxx = shutil.which("g++")
    if cxx is None:
        return None
    exe = Path(tempfile.mkdtemp(prefix="lbvh_reference_")) / "lbvh_reference"
    built = subprocess.run([cxx, "-std=c++20", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", str(SOURCE), "-o", str(exe)], capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    return exe


def reference_tree(scene):
    """The tree the serial restatement builds for `scene`: the dictionary of rt_amd.renderer.bvh_build (one row of `nodes` per
    node slot), plus `counts`."""
    exe = reference_binary()
    assert exe is not None, "no g++"
    g = bvh_cases.geometry_of(scene)
    with tempfile.TemporaryDirectory(prefix="lbvh_") as where:
        table, out = Path(where) / "table.bin", Path(where) / "tree.bin"
        table.write_bytes(np.uint32(len(g)).tobytes() + np.ascontiguousarray(g, dtype=np.float32).tobytes())
        done = subprocess.run([str(exe), str(table), str(out)], capture_output=True, text=True, timeout=120)
        assert done.returncode == 0, done.stderr
        raw = np.frombuffer(out.read_bytes(), dtype=np.uint32)
    counts = raw[:5].copy()
    n_nodes, n_tree, n_always, depth, root = (int(c) for c in counts)
    at = 5
    nodes = raw[at : at + 16 * n_nodes].view(np.float32).reshape(n_nodes, 16).copy()
    at += 16 * n_nodes
    order = raw[at : at + n_tree].copy()
    at += n_tree
    spheres = raw[at : at + 4 * n_tree].view(np.float32).reshape(n_tree, 4).copy()
    at += 4 * n_tree
    always = raw[at : at + n_always].copy()
    at += n_always
    bound = raw[at : at + 4].view(np.float32).copy()
    assert at + 4 == len(raw)
    return {"nodes": nodes, "order": order, "spheres": spheres, "always": always, "bound": bound, "depth": depth, "root": root, "counts": counts}


def same_bytes(a, b):
    """Two trees are the same bytes: counts, nodes, order, spheres, always, bound."""
    for key in ("nodes", "order", "spheres", "always", "bound"):
        x, y = np.ascontiguousarray(a[key]), np.ascontiguousarray(b[key])
        if x.shape != y.shape or not np.array_equal(x.view(np.uint32), y.view(np.uint32)):
            return False, key
    if (a["depth"], a["root"]) != (b["depth"], b["root"]):
        return False, "depth / root"
    return True, ""


# ---- scenes ---------------------------------------------------------------------------------------------------------------
def morton_staircase():
    """Clusters of five spheres at the origin, at 2^-j on each axis alone (j = 1 .. 10) and at (1, 1, 1): cluster (axis, j) owns
    the Morton cell with ONE bit set, so the highest differing bit peels off one cluster a level, thirty levels deep and more.
    bvh_cases.cluster_chain does not do that to this builder: 1024 cells an axis put its clusters from 16^-3 inwards into one
    cell, where the scene indices' bits cut them evenly (the model in tests/test_bvh_lbvh_reference.py says how deep)."""
    centres = [(0.0, 0.0, 0.0), (1.0, 1.0, 1.0)]
    for j in range(1, 11):
        for axis in range(3):
            c = [0.0, 0.0, 0.0]
            c[axis] = 2.0**-j
            centres.append(tuple(c))
    rows = np.zeros((len(centres) * 5, 5))
    for k, c in enumerate(centres):
        for m in range(5):
            rows[k * 5 + m] = (*c, 1e-4 * (1 + m), 0)
    return rows


def non_finite():
    rows = np.zeros((12, 5))
    rows[:, 3] = 0.5
    rows[0::3, 0] = np.nan
    rows[1::3, 3] = np.inf
    rows[2::3, 1] = -np.inf
    return rows


def field_rows(count):
    rows = np.asarray(bvh_cases.sphere_field(np.random.default_rng(1000 + count), count), dtype=np.float64)
    rows[:, 4] = 0  # (bvh_cases.sphere_scene has one material)
    return rows


@functools.lru_cache(maxsize=None)
def regime(name):
    return bvh_cases.regime_cases(name)


def scene_names():
    names = [f"field {n}" for n in (1, 4, 5, 8, 9, 300, 5000)]
    names += [f"regime {name}" for name in bvh_cases.REGIMES]
    names += ["always cap identical", "always cap distinct", "64 identical", "non-finite", "chain x", "chain y", "chain z", "morton staircase"]
    return names


def scenes_of(name):
    """The sphere rows (float64[n, 5]) a name stands for: one scene, or a regime's cases."""
    if name.startswith("field "):
        return [field_rows(int(name.split()[1]))]
    if name.startswith("regime "):
        return [rows for _, rows, _, _ in regime(name[len("regime ") :])]
    if name.startswith("chain "):
        return [bvh_cases.cluster_chain("xyz".index(name[-1]), 1.0)]
    if name.startswith("sized field "):
        return [sized_field_rows(int(name.split()[2]))]
    if name in SCALE_SPECIALS:
        return [SCALE_SPECIALS[name]()]
    return {
        "always cap identical": lambda: [bvh_cases.always_cap_identical()[0]],
        "always cap distinct": lambda: [bvh_cases.always_cap_distinct()[0]],
        "64 identical": lambda: [np.tile([(0.25, 0.5, -0.25, 0.125, 0)], (64, 1))],
        "non-finite": lambda: [non_finite()],
        "morton staircase": lambda: [morton_staircase()],
    }[name]()


# ---- scenes past one sort tile ----------------------------------------------------------------------------------------------
# The builder's launch constants (rt_amd/csrc/bvh_build.hip; tests/test_bvh_lbvh_reference.py reads them out of its text): the
# sizes below sit on the edges these make, so a retuned sort has to move the sizes with it.
THREADS, SORT_ROUNDS, SCAN_THREADS = 256, 16, 1024
SORT_TILE = THREADS * SORT_ROUNDS
DIGITS = 256  # histogram words a sort tile: 8 bits a pass

# n -> (sort tiles, trips of sort_scan's loop): what each size is there to reach
SIZED_FIELDS = {
    63: (1, 1), 64: (1, 1), 65: (1, 1), 255: (1, 1), 256: (1, 1), 257: (1, 1),  # wave and block edges of the per-sphere kernels and of sort_scatter's ballots
    4095: (1, 1), 4096: (1, 1), 4097: (2, 1), 8192: (2, 1), 8193: (3, 1),  # sort-tile edges
    12289: (4, 1), 16384: (4, 1),  # exactly 1024 histogram words: one full trip
    16385: (5, 2), 20481: (6, 2),  # the second trip, partial at 256 and at 512 words
    100000: (25, 7),  # the baseline's largest scene
    262145: (65, 17),
}


def sized_field_rows(count):
    """bvh_cases.sphere_field's distribution without its loop: the ground sphere first, radii 0.05 .. 0.3, x in +-12, z in -24 .. 0."""
    rng = np.random.default_rng(2000 + count)
    rows = np.zeros((count, 5))
    rows[0] = (0.0, -1000.0, 0.0, 1000.0, 0)
    r = rng.uniform(0.05, 0.3, count - 1)
    rows[1:, 0] = rng.uniform(-12.0, 12.0, count - 1)
    rows[1:, 1] = r
    rows[1:, 2] = rng.uniform(-24.0, 0.0, count - 1)
    rows[1:, 3] = r
    return rows


def one_cell(count=9000):
    """Identical spheres: the centres' extent is 0, so every sphere is large and the large sort runs over three tiles of equal
    keys; the tree's Morton codes are equal too.  The index alone decides both orders."""
    return np.tile([(0.25, 0.5, -0.25, 0.01, 0)], (count, 1))


def two_cells(count=9001):
    """x alternates between the two ends of the extent: no sphere is large, every wave of the sort holds two digits interleaved,
    and the order is the even indices, then the odd."""
    rows = one_cell(count)
    rows[1::2, 0] = 0.75
    return rows


def small_first(rows):
    """A field without its ground sphere (which is large): a sphere like the others in its place."""
    rows[0] = (0.0, 0.1, -12.0, 0.1, 0)
    return rows


def large_ties(count=9000):
    """80 large spheres anywhere in a field of three tiles, in 20 groups of 4 identical radii (8 .. 20; a quarter of the extent is
    6): the cap, 8 + 9000 / 256 = 43 = 10 * 4 + 3, cuts a group, and the cut goes to the group's lowest indices.
    Returns (rows, the large spheres' indices)."""
    rows = small_first(sized_field_rows(count))
    rng = np.random.default_rng(4300)
    large = rng.choice(np.arange(1, count), size=80, replace=False)
    radii = np.linspace(8.0, 20.0, 20) + rng.uniform(0.0, 0.5, 20)  # twenty distinct radii
    rows[large, 3] = np.repeat(radii, 4)[rng.permutation(80)]
    return rows, np.sort(large)


def large_near_cap(n_large, count=5000):
    """`n_large` large spheres of distinct radii anywhere in a field of two tiles whose cap is 8 + 5000 / 256 = 27."""
    rows = small_first(sized_field_rows(count))
    rng = np.random.default_rng(2700 + n_large)
    large = rng.choice(np.arange(1, count), size=n_large, replace=False)
    rows[large, 3] = rng.permutation(np.linspace(8.0, 20.0, n_large))
    return rows


def large_over_sixty_binades(count=6000):
    """Centres within 1e-20 of each other and radii log-uniform from 1e-19 to 2^40 (r^2 from 1e-38 to 2^80): every sphere is
    large and the large keys differ in all four digits.  Two pairs of equal radii, one of them at the cap's cut (31st largest)."""
    rng = np.random.default_rng(6000)
    rows = np.zeros((count, 5))
    rows[:, :3] = rng.uniform(-5e-21, 5e-21, (count, 3))
    rows[:, 3] = np.exp(rng.uniform(np.log(1e-19), np.log(2.0**39.99), count))
    by_size = np.argsort(-rows[:, 3], kind="stable")
    cap = 8 + count // 256
    rows[by_size[cap + 700], 3] = rows[by_size[cap - 1], 3]  # the cut's radius, once more outside the list
    rows[by_size[3000], 3] = rows[by_size[3001], 3]
    return rows


def mostly_non_finite(count=9000):
    """A field of three tiles with all but every 900th sphere made a NaN centre / an infinite radius / an infinite centre, as
    non_finite() does: a tree of nine (the ground sphere is large) under an always list of 8991, ascending."""
    rows = sized_field_rows(count)
    i = np.arange(count)
    gone = i % 900 != 0
    rows[gone & (i % 3 == 0), 0] = np.nan
    rows[gone & (i % 3 == 1), 3] = np.inf
    rows[gone & (i % 3 == 2), 1] = -np.inf
    return rows


SCALE_SPECIALS = {
    "one cell 9000": one_cell,
    "two cells 9001": two_cells,
    "large ties 9000": lambda: large_ties()[0],
    "large at the cap": lambda: large_near_cap(27),
    "large one above the cap": lambda: large_near_cap(28),
    "large over sixty binades": large_over_sixty_binades,
    "mostly non-finite 9000": mostly_non_finite,
}


def scale_names():
    """The scenes past one sort tile, beside scene_names() (the suites that walk every tree in Python hold them to fewer walks)."""
    return [f"sized field {n}" for n in SIZED_FIELDS] + list(SCALE_SPECIALS)


@functools.lru_cache(maxsize=None)
def scale_case(name):
    """(rows, scene, the restatement's tree) of one of scale_names(), made once for every test that asks; nobody writes to them."""
    (rows,) = scenes_of(name)
    scene = bvh_cases.sphere_scene(rows)
    tree = reference_tree(scene)
    for part in (rows, *(tree[key] for key in ("nodes", "order", "spheres", "always", "bound", "counts"))):
        part.setflags(write=False)
    return rows, scene, tree


def large_spheres(geometry):
    """The builder's rules `tame` and `large` (bvh_build.hpp) in numpy: (tame bool[n], large bool[n])."""
    g = np.asarray(geometry, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        tame = (g[:, 3] >= 0) & (g[:, 3] <= np.float32(2.0**80)) & (np.abs(g[:, :3]) <= np.float32(2.0**40)).all(axis=1)
    if not tame.any():
        return tame, tame.copy()
    c = g[tame, :3].astype(np.float64)
    extent = max(0.0, float((c.max(axis=0) - c.min(axis=0)).max()))
    with np.errstate(invalid="ignore"):
        return tame, tame & (np.sqrt(g[:, 3].astype(np.float64)) > extent / 4.0)


def level_widths(tree):
    """Inner nodes per level of a tree, the root's level first."""
    if len(tree["order"]) <= 4:
        return []
    links = tree["nodes"][:, [3, 7]].copy().view(np.uint32)
    widths, level = [], np.array([tree["root"]], dtype=np.uint32)
    while len(level):
        widths.append(len(level))
        below = links[level].reshape(-1)
        level = below[(below & np.uint32(0x80000000)) == 0]
    return widths


def reach(scene, tree):
    """What a scene makes the device builder do, from its size, its (c, r^2) table and the restatement's tree alone."""
    n = scene.n_spheres
    tame, large = large_spheres(bvh_cases.geometry_of(scene))
    cap = 8 + n // 256
    tiles = -(-n // SORT_TILE)
    widths = level_widths(tree)
    assert len(widths) == tree["depth"]
    taken = tree["always"][tame[tree["always"]]]  # the always list's large spheres (its others are not tame)
    assert len(taken) == min(int(large.sum()), cap) and large[taken].all()
    return {
        "n": n,
        "tiles": tiles,
        "scan trips": -(-DIGITS * tiles // SCAN_THREADS),
        "n_large": int(large.sum()),
        "cap": cap,
        "large sort runs": int(large.sum()) > cap,
        "always": len(tree["always"]),
        "always tiles": sorted(set((tree["always"] // SORT_TILE).tolist())),
        "taken tiles": sorted(set((taken // SORT_TILE).tolist())),
        "depth": tree["depth"],
        "widest level": max(widths, default=0),
        "level blocks at the bound": -(-(n // 5 + 1) // THREADS),
    }


# ---- the builder's keys and its cut without the depth cap, in numpy ---------------------------------------------------------
def spread3(v):
    v = v.astype(np.uint64)
    out = np.zeros_like(v)
    for bit in range(10):
        out |= ((v >> np.uint64(bit)) & np.uint64(1)) << np.uint64(3 * bit)
    return out


def model_keys(geometry, order):
    """(morton << 32 | scene index) of the tree's spheres, sorted: binary64 like bvh_build.hpp's morton30."""
    members = np.sort(order)
    c = geometry[members, :3].astype(np.float64)
    lo, hi = c.min(axis=0), c.max(axis=0)
    q = np.zeros(c.shape, dtype=np.uint64)
    for j in range(3):
        if hi[j] > lo[j]:
            t = (c[:, j] - lo[j]) / (hi[j] - lo[j]) * 1024.0
            q[:, j] = np.minimum(np.floor(t), 1023).astype(np.uint64)
    morton = (spread3(q[:, 0]) << np.uint64(2)) | (spread3(q[:, 1]) << np.uint64(1)) | spread3(q[:, 2])
    return np.sort((morton << np.uint64(32)) | members.astype(np.uint64))


def uncapped_depth(keys):
    """Inner-node levels of the tree that cuts every range of more than four sorted keys at its highest differing bit."""
    deepest, todo = 0, [(0, len(keys), 1)]
    while todo:
        first, count, level = todo.pop()
        if count <= 4:
            continue
        deepest = max(deepest, level)
        differing = int(keys[first]) ^ int(keys[first + count - 1])
        bit = np.uint64(1 << (differing.bit_length() - 1))
        cut = int(np.argmax((keys[first : first + count] & bit) != 0))
        assert 0 < cut < count
        todo += [(first, cut, level + 1), (first + cut, count - cut, level + 1)]
    return deepest
