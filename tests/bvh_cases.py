"""What the tests of RT_HIP_FLAG_BVH share (tests/test_bvh_build.py, tests/test_bvh_cull_audit.py on the CPU,
tests/test_gpu_bvh.py on the GPU): the structural check of a built tree, the scene and ray generators of every regime the
cull bound is a claim about, and a numpy binary32 restatement of the traversal's box test (bvh_scan.hpp, enter_box).

The restatement holds no sphere arithmetic: a sphere's distance always comes from the oracle.  The slab test is subtract,
add, multiply, one reciprocal and fmin / fmax, each of which numpy rounds as the device does."""
import numpy as np

import rt_amd
from oracle import binding as oracle

MATERIALS = [(0, 1, 1, 1, 1, 0.5, 0.5), (1, 0.9, 0.9, 0.9, 1, 0.1, 0.8), (0, 0.3, 0.6, 0.9, 1, 0.5, 0.5), (2, 1, 1, 1, 1, 0.0, 1.5), (1, 0.8, 0.6, 0.2, 1, 0.4, 0.8)]
LEAF = 0x80000000
STACK_DEPTH = 24  # bvh_max_depth (rt_amd/csrc/bvh.hpp)
MIN_HIT_DIST = 0.001  # min_hit_dist (rt_amd/csrc/contract.hpp): an absolute distance, whatever the scene's scale
F32 = np.float32


# ---- scenes and their trees -----------------------------------------------------------------------------------------------
def normalised(v):
    v = np.asarray(v, dtype=np.float64).reshape(-1, 3)
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def sphere_scene(rows):
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 5)
    return rt_amd.scene_from_arrays(spheres=rows, materials=[(0, 0.5, 0.5, 0.5, 1, 0, 0)])


def geometry_of(scene):
    n = scene.n_spheres
    c = [np.ctypeslib.as_array(p, (n,)).astype(np.float32) for p in (scene.sphere_center_x, scene.sphere_center_y, scene.sphere_center_z)]
    r = np.ctypeslib.as_array(scene.sphere_radius, (n,)).astype(np.float32)
    return np.stack(c + [r * r], axis=1).astype(np.float32)  # (cx, cy, cz, r^2) as the upload derives it


def leaf_range(link):
    return link & ((1 << 29) - 1), ((link >> 29) & 3) + 1


def check_tree(scene, t):
    n = scene.n_spheres
    g = geometry_of(scene)
    order, always, nodes = t["order"], t["always"], t["nodes"]
    # every sphere exactly once across the leaves and the always list
    assert np.array_equal(np.sort(np.concatenate([order, always])), np.arange(n, dtype=np.uint32))
    assert np.array_equal(always, np.sort(always))
    # the leaf table is a bit copy of the primitive table's rows
    assert np.array_equal(t["spheres"].view(np.uint32), g[order].view(np.uint32))
    assert t["depth"] <= STACK_DEPTH
    if len(order) == 0:
        return
    half = np.sqrt(g[:, 3].astype(np.float64))
    lo = g[:, :3].astype(np.float64) - half[:, None]
    hi = g[:, :3].astype(np.float64) + half[:, None]
    # the ball around the tree holds every tree sphere: |c - C| + sqrt(r^2) <= R
    centre, radius = t["bound"][:3].astype(np.float64), float(t["bound"][3])
    reach = np.linalg.norm(g[order, :3].astype(np.float64) - centre, axis=1) + half[order]
    assert (reach <= radius).all()
    links = nodes[:, [3, 7]].copy().view(np.uint32)
    seen_slots = np.zeros(len(order), dtype=np.int32)

    def walk(link, box_lo, box_hi, level):
        if link & LEAF:
            first, count = leaf_range(link)
            assert first + count <= len(order)
            seen_slots[first : first + count] += 1
            ids = order[first : first + count]
            if box_lo is not None:
                assert (lo[ids] >= box_lo).all() and (hi[ids] <= box_hi).all(), "a leaf box does not contain its spheres' boxes"
            return 0
        assert link < len(nodes)
        node = nodes[link].astype(np.float64)
        a_lo, a_hi, b_lo, b_hi = node[0:3], node[4:7], node[8:11], node[12:15]
        if box_lo is not None:
            assert (a_lo >= box_lo).all() and (a_hi <= box_hi).all() and (b_lo >= box_lo).all() and (b_hi <= box_hi).all(), "a node box does not contain its children's"
        return 1 + max(walk(int(links[link, 0]), a_lo, a_hi, level + 1), walk(int(links[link, 1]), b_lo, b_hi, level + 1))

    depth = walk(t["root"], None, None, 1)
    assert depth == t["depth"]
    assert (seen_slots == 1).all(), "every leaf slot belongs to exactly one leaf"
    # leaves of at most four spheres is what the link encodes; inner nodes number at most (tree spheres - 1)
    assert len(nodes) <= max(len(order) - 1, 0)


def sphere_field(rng, count, spread=12.0):
    spheres = [(0.0, -1000.0, 0.0, 1000.0, 0)]
    for _ in range(count - 1):
        r = rng.uniform(0.05, 0.3)
        spheres.append((rng.uniform(-spread, spread), r, rng.uniform(-2 * spread, 0), r, int(rng.integers(1, len(MATERIALS)))))
    return spheres


def adversarial_rays(spheres, rng, per_sphere=8):
    """Tangent and near-tangent rays (offsets of +-1..64 ulp of r from the tangent line), origins on and inside spheres."""
    origins, dirs = [], []
    s = np.asarray(spheres, dtype=np.float64)
    picks = rng.choice(len(s), size=min(len(s), 400), replace=False)
    for i in picks:
        c, r = s[i, :3].astype(np.float32).astype(np.float64), abs(float(np.float32(s[i, 3])))
        for k in range(per_sphere):
            d = rng.normal(size=3)
            d /= np.linalg.norm(d)
            side = np.cross(d, rng.normal(size=3))
            side /= np.linalg.norm(side)
            ulps = int(rng.choice([-64, -16, -4, -1, 0, 1, 4, 16, 64]))
            offset = r + ulps * float(np.spacing(np.float32(r)))
            dist = rng.uniform(0.5, 40.0)
            origins.append(c + side * offset - d * dist)  # tangent line at +-ulps
            dirs.append(d)
            if k % 2 == 0:  # an origin on the surface, as a bounce origin is, leaving outward or skimming
                n = rng.normal(size=3)
                n /= np.linalg.norm(n)
                origins.append(c + n * r)
                t = rng.normal(size=3)
                dirs.append(t / np.linalg.norm(t))
            else:  # inside
                origins.append(c + rng.normal(size=3) * r * 0.3)
                t = rng.normal(size=3)
                dirs.append(t / np.linalg.norm(t))
    return np.asarray(origins, dtype=np.float32), normalised(dirs)


# ---- the regimes ----------------------------------------------------------------------------------------------------------
# A regime is a list of cases (label, sphere rows float64[n, 5], origins float32[m, 3], directions float32[m, 3]); the CPU
# audit and the GPU comparison run the same cases.  "Spread" is the half-width of the cube the centres are drawn from.
def unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def log_uniform(rng, lo, hi, size):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), size))


def random_field(rng, count, r_lo=1e-4, r_hi=0.3):
    """Centres uniform in [-1, 1]^3 (spread 1), radii log-uniform in r_lo .. r_hi of the spread.  No sphere is large to the
    builder (radius above a quarter of the centres' extent, about 0.5), so every one is in the tree."""
    rows = np.zeros((count, 5))
    rows[:, :3] = rng.uniform(-1, 1, (count, 3))
    rows[:, 3] = log_uniform(rng, r_lo, r_hi, count)
    return rows


def rounded(rows):
    """Centres and radii as the scene holds them (binary32), in binary64."""
    return rows[:, :3].astype(F32).astype(np.float64), np.abs(rows[:, 3].astype(F32).astype(np.float64))


def tangent_rays(rows, rng, count, dist, targets=None, dirs=None):
    """adversarial_rays' first construction, vectorised: lines that pass a sphere at r +- 1..64 ulp of r, from `dist` (an
    array of `count` distances) before the tangent point.  `dirs`: directions to use instead of random ones."""
    c, r = rounded(rows)
    pick = rng.choice(len(rows) if targets is None else np.asarray(targets), size=count)
    d = unit(rng.normal(size=(count, 3))) if dirs is None else np.asarray(dirs, dtype=np.float64)
    side = np.cross(d, rng.normal(size=(count, 3)))
    side = unit(side)
    ulps = rng.choice([-64, -16, -4, -1, 0, 1, 4, 16, 64], size=count)
    offset = r[pick] + ulps * np.spacing(r[pick].astype(F32)).astype(np.float64)
    origins = c[pick] + side * offset[:, None] - d * np.asarray(dist)[:, None]
    return origins.astype(F32), (normalised(d) if dirs is None else np.asarray(dirs, dtype=F32))


def surface_and_inside_rays(rows, rng, count, targets=None):
    """adversarial_rays' other two constructions: origins on a sphere's surface (as a bounce origin is) and inside it."""
    c, r = rounded(rows)
    pick = rng.choice(len(rows) if targets is None else np.asarray(targets), size=count)
    on_surface = np.arange(count) % 2 == 0
    where = np.where(on_surface[:, None], unit(rng.normal(size=(count, 3))), rng.normal(size=(count, 3)) * 0.3)
    origins = c[pick] + where * r[pick, None]
    return origins.astype(F32), normalised(rng.normal(size=(count, 3)))


def near_rays(rows, rng, count, spread, targets=None):
    """Half tangents from 1e-3 .. 1e2 spreads away, half origins on and inside spheres."""
    o1, d1 = tangent_rays(rows, rng, count // 2, log_uniform(rng, 1e-3, 1e2, count // 2) * spread, targets)
    o2, d2 = surface_and_inside_rays(rows, rng, count - count // 2, targets)
    return np.concatenate([o1, o2]), np.concatenate([d1, d2])


def accepted_rays(rows, rng, count, targets=None):
    """Tangents from beyond min_hit_dist.  That distance is absolute (0.001), so in a scene a million times smaller no ray
    whose origin is a few spreads away has any hit at all: those scenes get these rays on top, from 0.0011 .. 1 away."""
    return tangent_rays(rows, rng, count, log_uniform(rng, 1.1 * MIN_HIT_DIST, 1.0, count), targets)


def scaled(rows, k):
    out = rows.copy()
    out[:, :4] = np.ldexp(rows[:, :4], k)
    return out


def regime_scale(rng):
    cases = []
    for k in (-60, -40, -20, 0, 20, 38):
        spread = 2.0**k
        rows = scaled(random_field(rng, 1500), k)
        o, d = near_rays(rows, rng, 20000, spread)
        if 1e2 * spread < 2 * MIN_HIT_DIST:  # nothing above can be accepted: twice as many rays that can
            o2, d2 = accepted_rays(rows, rng, 40000)
            o, d = np.concatenate([o, o2]), np.concatenate([d, d2])
        cases.append((f"2^{k}", rows, o, d))
    return cases


def regime_far(rng):
    rows = random_field(rng, 2000)
    o, d = tangent_rays(rows, rng, 100000, log_uniform(rng, 1e3, 1e6, 100000))
    return [("origins 1e3 .. 1e6 spreads away", rows, o, d)]


def regime_off_centre(rng):
    cases = []
    for shift in (1e3, 1e5, 1e6):
        rows = random_field(rng, 1500)
        rows[:, :3] += np.array([shift, -0.5 * shift, 0.25 * shift])
        o, d = near_rays(rows, rng, 34000, 1.0)
        cases.append((f"moved by {shift:g}", rows, o, d))
    return cases


def regime_underflow(rng):
    # r^2 = 2^-166 .. 2^-126 at r = 1e-25 .. 1e-19: zero below 2^-150, subnormal above
    rows = scaled(random_field(rng, 1500), -60)
    rows[:, 3] = log_uniform(rng, 1e-25, 1e-19, len(rows))
    r2 = rows[:, 3].astype(F32) * rows[:, 3].astype(F32)
    assert (r2 < np.finfo(F32).tiny).all() and (r2 == 0).any() and (r2 > 0).any()
    o, d = near_rays(rows, rng, 30000, 2.0**-60)
    o2, d2 = accepted_rays(rows, rng, 90000)
    return [("r^2 subnormal or zero", rows, np.concatenate([o, o2]), np.concatenate([d, d2]))]


def regime_duplicates(rng):
    rows = random_field(rng, 1500)
    src, dst = np.split(rng.choice(len(rows), size=300, replace=False), 2)
    rows[dst] = rows[src]  # a tenth of the spheres are now copies of others, anywhere in the index order
    o, d = near_rays(rows, rng, 100000, 1.0, targets=np.concatenate([src, dst]))
    return [("a tenth copied over others", rows, o, d)]


def axis_directions(rng, count):
    """Unit directions with one or two components exactly +0, -0, 1e-42 (subnormal: the reciprocal overflows) or 1e-30."""
    special = np.array([0.0, -0.0, 1e-42, -1e-42, 1e-30, -1e-30], dtype=F32)
    d = unit(rng.normal(size=(count, 3))).astype(F32)
    two = rng.random(count) < 0.4
    first = rng.integers(0, 3, count)
    second = (first + rng.integers(1, 3, count)) % 3
    rows = np.arange(count)
    d[rows, first] = 0
    d[rows[two], second[two]] = 0
    d = normalised(d)  # the components that are left: |d| = 1
    d[rows, first] = rng.choice(special, count)
    d[rows[two], second[two]] = rng.choice(special, two.sum())
    return d, first


def regime_axis(rng):
    rows = random_field(rng, 1500)
    tree = rt_amd.renderer.bvh_build(sphere_scene(rows))
    c, r = rounded(rows)
    count = 50000
    d, _ = axis_directions(rng, count)
    o1, d1 = tangent_rays(rows, rng, count, log_uniform(rng, 1e-3, 1e2, count), dirs=d)
    # origins with a coordinate EQUAL to a box face of the built tree, on an axis the ray does not move along (or barely):
    # the ray runs in that slab's plane, (face - o) is 0 and 0 * inf is a NaN.  The face is one that cuts the target sphere.
    d2, axis = axis_directions(rng, count)
    faces = tree["nodes"][:, [0, 1, 2, 4, 5, 6, 8, 9, 10, 12, 13, 14]].reshape(-1, 4, 3).astype(np.float64)
    pick = np.zeros(count, dtype=np.int64)
    face = np.zeros(count)
    for j in range(3):
        values = np.sort(faces[:, :, j].reshape(-1))
        first, last = np.searchsorted(values, c[:, j] - r), np.searchsorted(values, c[:, j] + r)
        cut = np.nonzero(last > first)[0]  # spheres some face cuts on this axis
        mine = np.nonzero(axis == j)[0]
        pick[mine] = rng.choice(cut, len(mine))
        face[mine] = values[first[pick[mine]] + (rng.random(len(mine)) * (last - first)[pick[mine]]).astype(np.int64)]
    rows_of = np.arange(count)
    inner = np.sqrt(np.maximum(r[pick] ** 2 - (face - c[pick, axis]) ** 2, 0.0))  # the circle the plane cuts out of the sphere
    aim = c[pick] + rng.uniform(-0.5, 0.5, (count, 3)) * inner[:, None]
    o2 = aim - d2.astype(np.float64) * (log_uniform(rng, 1e-3, 1e2, count) + r[pick])[:, None]
    o2 = o2.astype(F32)
    o2[rows_of, axis] = face.astype(F32)  # (faces are binary32 already)
    assert (o2[rows_of, axis].astype(np.float64) == face).all()
    return [("zero, subnormal and tiny components; origins on box faces", rows, np.concatenate([o1, o2]), np.concatenate([d1, d2]))]


REGIMES = {
    "scale sweep": regime_scale,
    "far origins": regime_far,
    "off-centre": regime_off_centre,
    "underflow": regime_underflow,
    "duplicates": regime_duplicates,
    "axis rays": regime_axis,
}


def regime_cases(name):
    """The cases of a regime: the same bytes wherever and whenever they are asked for."""
    return REGIMES[name](np.random.default_rng([7, list(REGIMES).index(name)]))


# ---- the builder's limits -------------------------------------------------------------------------------------------------
def cluster_chain(axis=0, sign=1.0):
    """Clusters of nine small spheres at 16^-i (1 + 0.01 j) along one axis, i = 0 .. 36, radius 0.001 * 16^-i.  Sixteen-bin
    SAH can peel off only the outermost cluster per level, so the builder's depth cap has to engage: depth 24 exactly."""
    rows = np.zeros((37 * 9, 5))
    for i in range(37):
        for j in range(9):
            rows[i * 9 + j, axis] = sign * 16.0**-i * (1 + 0.01 * j)
            rows[i * 9 + j, 3] = 0.001 * 16.0**-i
    return rows


def always_cap_identical():
    """20 spheres, 12 of them one identical large sphere: the always list takes 8 (its cap, 8 + n / 256), the lowest indices;
    4 copies stay in the tree, an exact tie in t between the list and the tree."""
    rows, large = np.zeros((20, 5)), [0, 2, 3, 5, 6, 7, 10, 11, 13, 16, 17, 19]
    small = [i for i in range(20) if i not in large]
    rows[large] = (0.25, 0.5, -0.25, 10.0, 0)
    for k, i in enumerate(small):
        rows[i] = (-1 + 2 * k / 7, 0.3 * (k % 3), 0.5 * (k % 2), 0.05, 0)
    return rows, large


def always_cap_distinct():
    """30 spheres, 12 of them large with distinct radii (in no order): the always list takes the 8 largest."""
    rows, large = np.zeros((30, 5)), [1, 4, 5, 8, 12, 13, 17, 20, 22, 25, 26, 29]
    radii = [7.0, 12.0, 5.5, 9.0, 16.0, 6.0, 11.0, 5.0, 14.0, 8.0, 15.0, 10.0]
    small = [i for i in range(30) if i not in large]
    for k, i in enumerate(large):
        rows[i] = (0.1 * k, -0.05 * k, 0.0, radii[k], 0)
    for k, i in enumerate(small):
        rows[i] = (-1 + 2 * k / 17, 0.3 * (k % 3), 0.5 * (k % 2), 0.05, 0)
    return rows, large, radii


# ---- the traversal's box test in numpy binary32 ---------------------------------------------------------------------------
def fused_dot(a, b):
    """dot() of contract.hpp, fma(a.z, b.z, fma(a.y, b.y, a.x * b.x)), through binary64: a product of two binary32 numbers is
    exact there, so each step is the exact sum rounded to binary64 and then to binary32 (the double rounding can differ from
    the fused result only on a tie to one part in 2^29: nothing a caller here decides by)."""
    a, b = np.asarray(a, dtype=F32).astype(np.float64), np.asarray(b, dtype=F32).astype(np.float64)
    with np.errstate(all="ignore"):
        s = (a[..., 0] * b[..., 0]).astype(F32).astype(np.float64)
        s = (a[..., 1] * b[..., 1] + s).astype(F32).astype(np.float64)
        return (a[..., 2] * b[..., 2] + s).astype(F32)


def query_pad(tree, origins, ulps, margin=2.0**-8):
    """pad = 2^-8 (|o - C| + R) + 2^-64 of bvh_scan.hpp, computed in binary64 from the binary32 o - C, rounded to binary32
    and stepped `ulps` ulp (negative: down).  The device rounds three times in the dot, once in the square root and once in
    each sum, at most 3.5 * 2^-24 in relative terms, which is less than 4 ulp: stepped -4 this pad is at most the device's,
    stepped +4 at least."""
    centre, radius = tree["bound"][:3].astype(F32), float(tree["bound"][3])
    oc = (np.asarray(origins, dtype=F32) - centre).astype(np.float64)
    with np.errstate(all="ignore"):
        pad = ((np.sqrt((oc * oc).sum(axis=-1)) + radius) * margin + 2.0**-64).astype(F32)
    for _ in range(abs(ulps)):
        pad = np.nextafter(pad, F32(-np.inf if ulps < 0 else np.inf))
    return pad


def enter_box(lo, hi, o, inv, pad, bound):
    """enter_box of bvh_scan.hpp on binary32 arrays (lo, hi, o, inv: [..., 3]; pad, bound: [...]): (entered, t_near, t_far)."""
    assert all(v.dtype == F32 for v in (lo, hi, o, inv, pad, bound))
    with np.errstate(all="ignore"):
        t0 = ((lo - o) - pad[..., None]) * inv
        t1 = ((hi - o) + pad[..., None]) * inv
        least, most = np.fmin(t0, t1), np.fmax(t0, t1)  # (fmin / fmax drop a NaN, as fminf / fmaxf do)
        t_near = np.fmax(np.fmax(least[..., 0], least[..., 1]), least[..., 2])
        t_far = np.fmin(np.fmin(most[..., 0], most[..., 1]), most[..., 2])
        return (t_near <= t_far + pad) & (t_near <= bound) & (t_far >= -pad), t_near, t_far


def reciprocal(d):
    with np.errstate(all="ignore"):
        return (F32(1.0) / np.asarray(d, dtype=F32)).astype(F32)


def gate_open(pad, dirs):
    """The two gates of bvh_spheres: a finite pad, and the computed |d|^2 within 2^-21 of 1."""
    dd = fused_dot(dirs, dirs)
    with np.errstate(all="ignore"):
        return (pad <= F32(2.0**100)) & (dd >= F32(1.0) - F32(2.0**-21)) & (dd <= F32(1.0) + F32(2.0**-21))


def root_paths(tree, n_spheres):
    """Per sphere of the tree: the boxes on the way from the root to its leaf.  (length int[n], lo float32[n, 24, 3], hi)."""
    nodes = tree["nodes"]
    links = nodes[:, [3, 7]].copy().view(np.uint32)
    length = np.zeros(n_spheres, dtype=np.int64)
    lo = np.zeros((n_spheres, STACK_DEPTH, 3), dtype=F32)
    hi = np.zeros((n_spheres, STACK_DEPTH, 3), dtype=F32)
    todo = [(int(tree["root"]), [])]
    while todo:
        link, path = todo.pop()
        if link & LEAF:
            first, count = leaf_range(link)
            for i in tree["order"][first : first + count]:
                length[i] = len(path)
                for level, (node, which) in enumerate(path):
                    lo[i, level] = nodes[node, which * 8 : which * 8 + 3]
                    hi[i, level] = nodes[node, which * 8 + 4 : which * 8 + 7]
        else:
            assert len(path) < STACK_DEPTH
            todo.append((int(links[link, 0]), path + [(link, 0)]))
            todo.append((int(links[link, 1]), path + [(link, 1)]))
    return length, lo, hi


def audit_cull(rows, origins, dirs, margin=2.0**-8):
    """Does the traversal cull a box between the root and the leaf of the sphere the oracle answers with?  With a pad at most
    the device's and bound = fl(t + pad), the tightest the traversal can hold while that sphere is still to be found; every
    operation of enter_box is monotone in both, so a box that passes here is entered on the device.  Returns the counts and
    the least slack seen, min(bound - t_near, t_far + pad, t_far + pad - t_near) / pad."""
    scene = sphere_scene(rows)
    tree = rt_amd.renderer.bvh_build(scene)
    t, kind, index, _ = oracle.closest_hit(scene, origins, dirs)
    in_tree = np.zeros(len(rows), dtype=bool)
    in_tree[tree["order"]] = True
    pad = query_pad(tree, origins, -4, margin)
    hit = kind == 1
    excluded = ~gate_open(query_pad(tree, origins, 0), dirs) | (hit & ~np.isfinite(t))
    answered = hit & in_tree[np.where(hit, index, 0)] & ~excluded
    result = {"rays": len(origins), "answered": int(answered.sum()), "excluded": int(excluded.sum()), "culled": 0, "slack": np.inf, "depth": tree["depth"], "tree": len(tree["order"])}
    if not answered.any():
        return result
    length, lo, hi = root_paths(tree, len(rows))
    o, d, t, i, pad = origins[answered].astype(F32), dirs[answered].astype(F32), t[answered], index[answered], pad[answered]
    bound = (t + pad).astype(F32)
    levels = length[i].max()
    shape = (len(o), levels, 3)
    entered, t_near, t_far = enter_box(lo[i, :levels], hi[i, :levels], np.broadcast_to(o[:, None], shape), np.broadcast_to(reciprocal(d)[:, None], shape), np.broadcast_to(pad[:, None], shape[:2]), np.broadcast_to(bound[:, None], shape[:2]))
    real = np.arange(levels)[None, :] < length[i][:, None]
    result["culled"] = int((real & ~entered).sum())
    if result["culled"]:
        ray, level = np.argwhere(real & ~entered)[0]
        result["first"] = f"o={o[ray]} d={d[ray]} t={t[ray]} sphere {i[ray]} level {level} pad={pad[ray]} t_near={t_near[ray, level]} t_far={t_far[ray, level]}"
    with np.errstate(all="ignore"):
        near64, far64, pad64 = t_near.astype(np.float64), t_far.astype(np.float64), pad.astype(np.float64)[:, None]
        slack = np.minimum(np.minimum(bound.astype(np.float64)[:, None] - near64, far64 + pad64), far64 + pad64 - near64) / pad64
    result["slack"] = float(np.where(real, slack, np.inf).min())
    return result


# ---- the visiting order, for the few rays of the full-stack tests ----------------------------------------------------------
def leaf_answers(rows, tree, origins, dirs):
    """Per leaf link: the oracle's (t, scene index) of each ray against that leaf's spheres alone (t NaN where it misses).
    For finite distances the oracle's sequential rule over spheres in index order is the minimum of (t, index)."""
    out = {}
    todo = [int(tree["root"])]
    links = tree["nodes"][:, [3, 7]].copy().view(np.uint32)
    while todo:
        link = todo.pop()
        if link & LEAF:
            first, count = leaf_range(link)
            ids = np.sort(tree["order"][first : first + count])
            t, kind, index, _ = oracle.closest_hit(sphere_scene(rows[ids]), origins, dirs)
            out[link] = (np.where(kind == 1, t, F32(np.nan)), ids[np.where(kind == 1, index, 0)])
        else:
            todo += [int(links[link, 0]), int(links[link, 1])]
    return out


def model_traversal(rows, tree, origin, direction, ray, answers, pad):
    """bvh_spheres' walk for one ray (no always list): (t or None, index, the most stack entries in use at once)."""
    nodes = tree["nodes"]
    links = nodes[:, [3, 7]].copy().view(np.uint32)
    o, inv, pad = np.asarray(origin, dtype=F32), reciprocal(direction), F32(pad)
    best_t, best_i = None, 0
    stack, deepest, link = [], 0, int(tree["root"])
    while True:
        descended = False
        if link & LEAF:
            t, i = answers[link][0][ray], int(answers[link][1][ray])
            if not np.isnan(t) and (best_t is None or t < best_t or (t == best_t and i < best_i)):
                best_t, best_i = t, i
        else:
            bound = F32(np.inf) if best_t is None else F32(best_t + pad)
            in_a, near_a, _ = enter_box(nodes[link, 0:3], nodes[link, 4:7], o, inv, pad, bound)
            in_b, near_b, _ = enter_box(nodes[link, 8:11], nodes[link, 12:15], o, inv, pad, bound)
            link_a, link_b = int(links[link, 0]), int(links[link, 1])
            if in_a and in_b:
                a_first = near_a <= near_b
                stack.append(link_b if a_first else link_a)
                deepest = max(deepest, len(stack))
                link, descended = (link_a if a_first else link_b), True
            elif in_a or in_b:
                link, descended = (link_a if in_a else link_b), True
        if descended:
            continue
        if not stack:
            return best_t, best_i, deepest
        link = stack.pop()
