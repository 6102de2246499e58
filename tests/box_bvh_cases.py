"""What the tests of RT_HIP_FLAG_BOX_BVH share (tests/test_box_bvh_build.py and tests/test_box_bvh_cull_audit.py on the CPU,
tests/test_gpu_box_bvh.py on the GPU): scenes of boxes, the structural check of a built tree, the chain that drives the builder to
its depth limit, ray generators, and a numpy binary32 restatement of the traversal's node test and gate (box_bvh_scan.hpp:
enter_node, box_bvh_takes).  TEST INFRASTRUCTURE.

The restatement holds no box arithmetic of its own beyond that node test: a box's distance always comes from
tests/native/box_reference.cpp.  The node test is subtract, multiply, one reciprocal and compare-and-select, each of which numpy
rounds as the device does."""
import functools

import numpy as np

import rt_amd
from tests import box_reference as box_ref
from tests.bvh_cases import LEAF, STACK_DEPTH, leaf_range

F32 = np.float32
KIND_BOX = box_ref.KIND_BOX


@functools.lru_cache(maxsize=None)
def camera(width=64, height=36):
    return rt_amd.Scene.named("basic").describe(width, height)


def box_scene(boxes, spheres=(), planes=(), spp=16, bounces=6, size=(64, 36)):
    """boxes: rows (cx, cy, cz, ex, ey, ez, material) — see box_reference.scene_pod."""
    return box_ref.scene_pod(camera(*size), spheres=spheres, planes=planes, boxes=[tuple(b) for b in boxes], spp=spp, bounces=bounces)


def bounds_of(scene):
    """The pairs as the upload derives them: float32[n, 8] = (c - e, material bits, c + e, 0)."""
    n = scene.n_boxes
    out = np.zeros((n, 8), dtype=F32)
    if n == 0:
        return out
    c = np.stack([np.ctypeslib.as_array(p, (n,)).astype(F32) for p in (scene.box_center_x, scene.box_center_y, scene.box_center_z)], axis=1)
    e = np.stack([np.ctypeslib.as_array(p, (n,)).astype(F32) for p in (scene.box_extents_x, scene.box_extents_y, scene.box_extents_z)], axis=1)
    with np.errstate(all="ignore"):
        out[:, 0:3] = c - e
        out[:, 4:7] = c + e
    out[:, 3] = np.ctypeslib.as_array(scene.box_material, (n,)).astype(np.uint32).view(F32)
    return out


def extents_of(bounds):
    """Per-axis min and max of the two corners (NaN rows are not in a tree)."""
    with np.errstate(all="ignore"):
        return np.minimum(bounds[:, 0:3], bounds[:, 4:7]), np.maximum(bounds[:, 0:3], bounds[:, 4:7])


def check_box_tree(scene, t):
    """Every box once, leaf slots bit copies, child boxes the EXACT unions of what lies below them, depth within the stack."""
    n = scene.n_boxes
    bounds = bounds_of(scene)
    order, always, nodes = t["order"], t["always"], t["nodes"]
    assert np.array_equal(np.sort(np.concatenate([order, always])), np.arange(n, dtype=np.uint32)), "every box exactly once, in a leaf slot or in the always list"
    assert np.array_equal(always, np.sort(always))
    assert np.array_equal(t["corners"].view(np.uint32), bounds[order].view(np.uint32)), "leaf slots are bit copies of the uploaded pairs"
    finite = np.isfinite(bounds[:, [0, 1, 2, 4, 5, 6]]).all(axis=1)
    assert finite[order].all(), "a box with a non-finite corner is in the tree"
    assert set(np.flatnonzero(~finite).tolist()) <= set(always.tolist())
    assert t["depth"] <= STACK_DEPTH
    if len(order) == 0:
        assert len(nodes) == 0
        return
    lo, hi = extents_of(bounds)
    links = nodes[:, [3, 7]].copy().view(np.uint32)
    seen_slots = np.zeros(len(order), dtype=np.int32)

    def walk(link):
        """(union lo, union hi, inner levels) of the subtree."""
        if link & LEAF:
            first, count = leaf_range(link)
            assert 1 <= count <= 4 and first + count <= len(order)
            seen_slots[first : first + count] += 1
            ids = order[first : first + count]
            return lo[ids].min(axis=0), hi[ids].max(axis=0), 0
        assert link < len(nodes)
        node = nodes[link]
        a = walk(int(links[link, 0]))
        b = walk(int(links[link, 1]))
        assert node[0:3].tobytes() == a[0].tobytes() and node[4:7].tobytes() == a[1].tobytes(), "child box A is not the exact union of what lies below it"
        assert node[8:11].tobytes() == b[0].tobytes() and node[12:15].tobytes() == b[1].tobytes(), "child box B is not the exact union of what lies below it"
        return np.minimum(a[0], b[0]), np.maximum(a[1], b[1]), 1 + max(a[2], b[2])

    assert walk(t["root"])[2] == t["depth"]
    assert (seen_slots == 1).all(), "every leaf slot belongs to exactly one leaf"
    assert len(nodes) <= max(len(order) - 1, 0)


def build_twice(scene):
    a, b = rt_amd.renderer.box_bvh_build(scene), rt_amd.renderer.box_bvh_build(scene)
    for key in ("nodes", "order", "corners", "always"):
        assert a[key].tobytes() == b[key].tobytes(), f"two builds differ in {key}"
    assert (a["depth"], a["root"]) == (b["depth"], b["root"])
    return a


def camera_at(position, direction, width=64, height=36):
    return rt_amd.Scene.named("basic").set_camera(position, direction).describe(width, height)


# ---- scenes -------------------------------------------------------------------------------------------------------------------
def grid_boxes(count, pitch=0.3, half=0.1, y=0.1, z0=0.0, materials=4):
    side = int(np.ceil(np.sqrt(count)))
    return [((i % side - side / 2) * pitch, y + 0.05 * (i % 3), z0 - (i // side) * pitch, half, y + 0.05 * (i % 3), half, i % materials) for i in range(count)]


def chain_boxes(axis=0, sign=1.0):
    """Clusters of nine small boxes at 16^-i (1 + 0.01 j) along one axis, i = 0 .. 36, half width 0.001 * 16^-i (bvh_cases.cluster_chain
    with boxes).  Sixteen-bin SAH can peel off only the outermost cluster per level, so the depth cap has to engage: depth 24."""
    rows = np.zeros((37 * 9, 7))
    for i in range(37):
        for j in range(9):
            rows[i * 9 + j, axis] = sign * 16.0**-i * (1 + 0.01 * j)
            rows[i * 9 + j, 3:6] = 0.001 * 16.0**-i
    return rows


def random_boxes(rng, count, spread=4.0, e_lo=1e-3, e_hi=0.4, nested=0):
    """Random boxes in a cube of side 2 * spread; `nested` of them are shells around the origin of growing size."""
    rows = np.zeros((count, 7))
    rows[:, 0:3] = rng.uniform(-spread, spread, (count, 3))
    rows[:, 3:6] = np.exp(rng.uniform(np.log(e_lo), np.log(e_hi), (count, 3)))
    rows[:, 6] = rng.integers(0, 4, count)
    for k in range(nested):
        rows[k, 0:3] = rng.uniform(-0.01, 0.01, 3)
        rows[k, 3:6] = 0.2 * (k + 1) * rng.uniform(0.9, 1.1, 3)
    return rows.astype(F32).astype(np.float64)  # (values binary32 holds: scaling by a power of two below keeps every rounding)


def scaled(rows, k):
    rows = np.array(rows, dtype=np.float64)
    rows[:, 0:6] *= k
    return rows


def unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def rays_at(rows, rng, count, scale=1.0):
    """Origins on faces, on edges, inside boxes (the nested ones among them), far away and along an axis, aimed at boxes; float32."""
    rows = np.asarray(rows, dtype=np.float64)
    lo, hi = rows[:, 0:3] - np.abs(rows[:, 3:6]), rows[:, 0:3] + np.abs(rows[:, 3:6])
    pick = rng.integers(0, len(rows), count)
    aim = rng.integers(0, len(rows), count)
    u = rng.uniform(0, 1, (count, 3))
    inside = lo[pick] + u * (hi[pick] - lo[pick])
    origins = inside.copy()
    how = rng.integers(0, 5, count)
    face_axis = rng.integers(0, 3, count)
    side = rng.integers(0, 2, count)
    on_face = how == 0
    origins[on_face, face_axis[on_face]] = np.where(side[on_face] == 0, lo[pick[on_face], face_axis[on_face]], hi[pick[on_face], face_axis[on_face]])
    on_edge = how == 1
    for shift in (0, 1):
        ax = (face_axis + shift) % 3
        origins[on_edge, ax[on_edge]] = np.where(side[on_edge] == 0, lo[pick[on_edge], ax[on_edge]], hi[pick[on_edge], ax[on_edge]])
    far = how == 3
    origins[far] = unit(rng.normal(size=(int(far.sum()), 3))) * scale * 10.0 ** rng.uniform(1, 4, (int(far.sum()), 1))
    target = lo[aim] + rng.uniform(0, 1, (count, 3)) * (hi[aim] - lo[aim])
    d = target - origins
    d[np.linalg.norm(d, axis=1) == 0] = (0.0, 0.0, -1.0)
    d = unit(d)
    # ... and along an axis from beyond min_hit_dist, whatever the scene's scale (a scene of 2^-60 cannot be aimed at from 0.001 away: a
    # direction has 24 bits): the origin is the target moved down one axis, the other two components tiny, of finite reciprocal
    along = np.flatnonzero(how == 4)
    axis = rng.integers(0, 3, len(along))
    sign = np.where(rng.integers(0, 2, len(along)) == 0, -1.0, 1.0)
    reach = 10.0 ** rng.uniform(-2.5, 2, len(along)) + 10.0 * scale
    origins[along] = target[along]
    origins[along, axis] = target[along, axis] - sign * reach
    d[along] = np.where(rng.integers(0, 2, (len(along), 3)) == 0, -1.0, 1.0) * 2.0 ** rng.uniform(-100, -60, (len(along), 3))
    d[along, axis] = sign
    return origins.astype(F32), d.astype(F32)


def degenerate_directions(rng, count):
    """Directions with one or two components that are +0, -0, subnormal, tiny (their reciprocal finite and huge) or so small that the
    reciprocal overflows; the rest of ordinary size.  Normalised where that keeps the special value."""
    d = unit(rng.normal(size=(count, 3)))
    specials = np.array([0.0, -0.0, 1e-45, -1e-45, 3e-39, -3e-39, 2.0**-126, -(2.0**-126), 2.0**-100, -(2.0**-100), 1e-30, -1e-30, 2.0**-127, 1e-20])
    for axis in range(2):
        ax = rng.integers(0, 3, count)
        use = rng.integers(0, 3, count) > axis
        d[np.flatnonzero(use), ax[use]] = 0.0
    d = unit(np.where(np.abs(d).sum(axis=1, keepdims=True) == 0, (0.0, 0.0, 1.0), d))
    out = d.astype(F32)
    zero = out == 0
    out[zero] = specials[rng.integers(0, len(specials), int(zero.sum()))].astype(F32)
    return out


# ---- the node test and the gate, binary32 ---------------------------------------------------------------------------------------
def reciprocal(d):
    with np.errstate(all="ignore"):
        return (F32(1.0) / np.asarray(d, dtype=F32)).astype(F32)


def select_min(a, b):
    return np.where(a < b, a, b)


def select_max(a, b):
    return np.where(a > b, a, b)


def slabs(lo, hi, o, inv):
    """hits_box_given's tmin and tmax of the box [lo, hi] (any leading shape, last axis 3), binary32 throughout."""
    with np.errstate(all="ignore"):
        t1 = ((lo.astype(F32) - o.astype(F32)).astype(F32) * inv.astype(F32)).astype(F32)
        t2 = ((hi.astype(F32) - o.astype(F32)).astype(F32) * inv.astype(F32)).astype(F32)
        near, far = select_min(t1, t2), select_max(t1, t2)
        tmin = select_max(select_max(near[..., 0], near[..., 1]), near[..., 2])
        tmax = select_min(select_min(far[..., 0], far[..., 1]), far[..., 2])
    return tmin, tmax


def enter_node(lo, hi, o, inv, best_t):
    """enter_node with a best candidate at best_t: the comparisons written the device's way round."""
    tmin, tmax = slabs(lo, hi, o, inv)
    with np.errstate(all="ignore"):
        return ~(tmax < tmin) & ~(tmax < F32(0.0)) & ~(tmin > best_t), tmin, tmax


def gate_takes(origins, dirs):
    """box_bvh_takes: every reciprocal finite and not zero, the origin finite."""
    inv = reciprocal(dirs)
    with np.errstate(all="ignore"):
        return (np.isfinite(inv) & (inv != 0)).all(axis=1) & np.isfinite(np.asarray(origins, dtype=F32)).all(axis=1)


def root_paths(tree, n_boxes):
    """Per box of the tree: the child boxes on the way from the root to its leaf.  (length int[n], lo float32[n, 24, 3], hi)."""
    nodes = tree["nodes"]
    links = nodes[:, [3, 7]].copy().view(np.uint32)
    length = np.zeros(n_boxes, dtype=np.int64)
    lo = np.zeros((n_boxes, STACK_DEPTH, 3), dtype=F32)
    hi = np.zeros((n_boxes, STACK_DEPTH, 3), dtype=F32)
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


def audit_cull(rows, origins, dirs, rng):
    """Does the traversal skip a node between the root and the leaf of the box the restatement answers with?  With best.t = the
    answer's own t, the tightest the traversal can hold while that box is still to be found.  Also the lemma the cull rests on, for
    one random tree box per ray whether it is hit or not: tmin_N <= tmin_b and tmax_N >= tmax_b on every node above it."""
    scene = box_scene(rows)
    tree = rt_amd.renderer.box_bvh_build(scene)
    t, kind, index, _ = box_ref.closest_hit(scene, origins, dirs)
    in_tree = np.zeros(len(rows), dtype=bool)
    in_tree[tree["order"]] = True
    takes = gate_takes(origins, dirs)
    hit = kind == KIND_BOX
    answered = hit & in_tree[np.where(hit, index, 0)] & takes
    result = {"rays": len(origins), "taken": int(takes.sum()), "answered": int(answered.sum()), "skipped": 0, "lemma_broken": 0, "depth": tree["depth"], "tree": len(tree["order"])}
    if len(tree["order"]) == 0:
        return result
    length, lo, hi = root_paths(tree, len(rows))
    inv = reciprocal(dirs)
    o32 = np.asarray(origins, dtype=F32)
    if answered.any():
        o, v, ta, i = o32[answered], inv[answered], t[answered], index[answered]
        levels = max(int(length[i].max()), 1)
        shape = (len(o), levels, 3)
        entered, _, _ = enter_node(lo[i, :levels], hi[i, :levels], np.broadcast_to(o[:, None], shape), np.broadcast_to(v[:, None], shape), ta[:, None])
        real = np.arange(levels)[None, :] < length[i][:, None]
        result["skipped"] = int((real & ~entered).sum())
        if result["skipped"]:
            ray, level = np.argwhere(real & ~entered)[0]
            result["first"] = f"o={o[ray]} inv={v[ray]} t={ta[ray]} box {i[ray]} level {level}"
    if takes.any():
        bounds = bounds_of(scene)
        o, v = o32[takes], inv[takes]
        i = tree["order"][rng.integers(0, len(tree["order"]), len(o))]
        levels = max(int(length[i].max()), 1)
        shape = (len(o), levels, 3)
        tmin_b, tmax_b = slabs(bounds[i, 0:3], bounds[i, 4:7], o, v)
        tmin_n, tmax_n = slabs(lo[i, :levels], hi[i, :levels], np.broadcast_to(o[:, None], shape), np.broadcast_to(v[:, None], shape))
        real = np.arange(levels)[None, :] < length[i][:, None]
        assert not (np.isnan(tmin_b).any() or np.isnan(tmax_b).any() or np.isnan(tmin_n[real]).any() or np.isnan(tmax_n[real]).any()), "a NaN behind the gate"
        broken = real & ~((tmin_n <= tmin_b[:, None]) & (tmax_n >= tmax_b[:, None]))
        result["lemma_broken"] = int(broken.sum())
    return result


def model_stack_depth(tree, bounds, origin, direction):
    """The deepest the lane's stack gets for one ray the gate takes: bvh_boxes restated for the visiting order alone (the nearer
    child first, the other waits), binary32.  Which box wins is not taken from here."""
    o, inv = np.asarray(origin, dtype=F32), reciprocal(np.asarray(direction, dtype=F32))
    nodes = tree["nodes"]
    links = nodes[:, [3, 7]].copy().view(np.uint32)
    best = None  # (t, index)
    link, stack, deepest = int(tree["root"]), [], 0
    while True:
        if link & LEAF:
            first, count = leaf_range(link)
            for slot in range(first, first + count):
                i = int(tree["order"][slot])
                tmin, tmax = slabs(bounds[i, 0:3], bounds[i, 4:7], o, inv)
                if tmax >= tmin and not tmax < 0:
                    t = tmin if tmin >= 0 else tmax
                    if not t < F32(0.001) and (best is None or (t, i) < best):
                        best = (t, i)
        else:
            entered = []
            for which in (0, 1):
                tmin, tmax = slabs(nodes[link, which * 8 : which * 8 + 3], nodes[link, which * 8 + 4 : which * 8 + 7], o, inv)
                entered.append((not tmax < tmin and not tmax < 0 and not (best is not None and tmin > best[0]), tmin))
            if entered[0][0] and entered[1][0]:
                a_first = entered[0][1] <= entered[1][1]
                stack.append(int(links[link, 1 if a_first else 0]))
                deepest = max(deepest, len(stack))
                link = int(links[link, 0 if a_first else 1])
                continue
            if entered[0][0] or entered[1][0]:
                link = int(links[link, 0 if entered[0][0] else 1])
                continue
        if not stack:
            return deepest
        link = stack.pop()
