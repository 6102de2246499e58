"""The float64 numpy restatement of the mg / sm path (see tests/test_independent_path_tracer.py, which holds the oracle to it), shared,
and with one hook: an ENSEMBLE of perturbed runs that says, per pixel, what float32-sized errors can do to it.

`trace(pod, width, height, seed, runs=[Run, ...])` traces all runs in one numpy pass — the runs are an extra lane axis in front of the
(pixel, sample) lanes, fed the same random streams.  In a run of amplitude `a` every intermediate that float32 code rounds is multiplied by
1 + a * 2^-23 * r, r uniform in [-1, 1] from the batch's seeded generator: the primary direction; the dots n.d, n.o, e.d, e.e; e2 - a^2, the
root f, every t, the hit position, the outward normal, the unit-vector draw; normal + unit, dot(shiny, normal) and the normalised scatter
direction.  (All of them: with only the roots, quotients and normalisations perturbed the float32 oracle flipped samples that no run had.)

`allowance(case)` is the per-pixel rule RT_HIP_FLAG_FAST's builds are held to (tests/fast_cases.py has the cases and the constants):
    base      = the unperturbed float64 mean
    spread    = max over R runs at amplitude A of |run - base|, per pixel (largest channel)
    allowance = 2e-5 * scale + 2 * spread,   scale = max(|base| over channels, 1e-6)
A pixel none of whose samples sits near a decision has a spread of rounding size and is held to 2e-5 relative (tests/test_gpu_fast.py's own
rounding tolerance); a pixel with a sample that can fall the other way has seen it fall in some run, and is widened by what that changes.

Two deliberately WRONG runs exist for the teeth of the rule: `unit_scale` scales the unit-vector draw, `shift_last` draws each pixel's last
sample from the next sample index's stream."""
import dataclasses

import numpy as np

from tests.test_oracle_kat import M32, _STEP_MULTIPLIERS, _stream_start

MIN_HIT_DIST = 0.001  # mg_ray_tracer.cpp:20
APPROX_ZERO = 1.0e-6  # muu's default epsilon for float (vector::approx_zero)
METAL = 1  # material_type::metal, src/common.hpp:105-115
REFRACTING = (2, 3, 4, 5, 6)  # dielectric, air, vacuum, water, ice: sm_ray_tracer.cpp:229-233
ULP = 2.0**-23

ROUNDING = 2e-5  # tests/test_gpu_fast.py: what rounding alone may move a pixel's mean by, relative to `scale`
SCALE_FLOOR = 1e-6
SPREAD_FACTOR = 2.0
TIGHT = 1e-4  # a pixel whose allowance is at most this (relative to scale) is TIGHT: held to rounding


@dataclasses.dataclass(frozen=True)
class Run:
    amplitude: float = 0.0  # float32 ulps
    unit_scale: float = 1.0  # wrong variant (a): the unit-vector draw times this
    shift_last: bool = False  # wrong variant (b): each pixel's last sample from the next sample index's stream


EXACT = Run()


def column(pointer, n, dtype=np.float64):
    return np.array([pointer[i] for i in range(n)], dtype=dtype)


class Streams:
    """one random stream per (pixel, sample): contract v4, numpy (tests/test_oracle_kat.py::_draws, one generator step at a time).
    A step serves one call of random<T>() and yields up to three numbers (src/random.hpp:37-46: components in brace-init order)."""

    def __init__(self, seed, pixels, samples):
        self.key, self.stride, self.counter = _stream_start(seed, pixels, samples)

    def step(self, lanes, components):
        c = (self.counter[lanes] + self.stride[lanes]) & M32
        self.counter[lanes] = c
        x = c ^ (c >> np.uint64(16))
        x = (x * np.uint64(0x7FEB352D) + self.key[lanes]) & M32
        x ^= x >> np.uint64(15)
        return np.stack([(((x * m) & M32) >> np.uint64(8)).astype(np.float64) * 2.0**-24 for m in _STEP_MULTIPLIERS[:components]], axis=-1)

    def next(self, lanes):
        """random<float>()"""
        return self.step(lanes, 1)[:, 0]

    def unit_vector(self, lanes):
        """random_unit_vector(), src/random.hpp:57-66: x, y, z in [0, 1), normalised (all zero: 2^-72, not handled here)"""
        v = self.step(lanes, 3)
        return v / np.linalg.norm(v, axis=-1, keepdims=True)


def trace(pod, width, height, seed, sm_materials=False, runs=(EXACT,), noise_seed=0):
    """float64 mean colour per run and pixel, [len(runs), height, width, 3], and `bounced`, bool [len(runs), height, width]: a sample of
    the pixel hit something."""
    spp, max_bounces = pod.samples_per_pixel, pod.max_bounces
    centres = np.stack([column(pod.sphere_center_x, pod.n_spheres), column(pod.sphere_center_y, pod.n_spheres), column(pod.sphere_center_z, pod.n_spheres)], axis=-1)
    radii = column(pod.sphere_radius, pod.n_spheres)
    sphere_material = column(pod.sphere_material, pod.n_spheres, np.int64)
    plane_n = np.stack([column(pod.plane_normal_x, pod.n_planes), column(pod.plane_normal_y, pod.n_planes), column(pod.plane_normal_z, pod.n_planes)], axis=-1)
    plane_d = column(pod.plane_d, pod.n_planes)
    plane_material = column(pod.plane_material, pod.n_planes, np.int64)
    kind = column(pod.material_type, pod.n_materials, np.int64)
    albedo = column(pod.material_albedo, 4 * pod.n_materials).reshape(-1, 4)[:, :3]  # rt::colour: r, g, b, a per material (src/colour.hpp:17-57)
    attenuation_of = albedo * column(pod.material_reflectivity, pod.n_materials)[:, None]  # :115,131
    roughness = column(pod.material_roughness, pod.n_materials)
    reflectivity = column(pod.material_reflectivity, pod.n_materials)
    inverse_vp = np.array(list(pod.inverse_view_projection), dtype=np.float64).reshape(4, 4)

    n_runs = len(runs)
    rs, ys, xs, ss = np.meshgrid(np.arange(n_runs), np.arange(height), np.arange(width), np.arange(spp), indexing="ij")
    rs, xs, ys, ss = rs.ravel(), xs.ravel(), ys.ravel(), ss.ravel()
    n = xs.size
    amplitude = np.array([r.amplitude for r in runs], dtype=np.float64)[rs] * ULP
    unit_scale = np.array([r.unit_scale for r in runs], dtype=np.float64)[rs]
    shifted = np.array([r.shift_last for r in runs], dtype=bool)[rs] & (ss == spp - 1)
    noisy = bool(amplitude.any())
    noise = np.random.default_rng(noise_seed)

    def rounded(value, lanes):
        """the hook: `value` (of lanes `lanes`, scalars or vectors) as a float32 computation of the run's error size might have left it"""
        if not noisy:
            return value
        a = amplitude[lanes]
        return value * (1.0 + (a if value.ndim == 1 else a[:, None]) * noise.uniform(-1.0, 1.0, value.shape))

    stream_sample = ss + shifted
    streams = Streams(seed, (ys * width + xs).astype(np.uint32), stream_sample.astype(np.uint32))
    everyone = np.arange(n)
    # `pos = screen_pos + (i ? random<vec2>() : vec2{0.5})` (:189): sample 0 draws nothing here
    later = everyone[stream_sample > 0]
    jitter_x, jitter_y = np.full(n, 0.5), np.full(n, 0.5)
    jitter = streams.step(later, 2)  # random<vec2>()
    jitter_x[later], jitter_y[later] = jitter[:, 0], jitter[:, 1]
    px, py = xs + jitter_x, ys + jitter_y

    def screen_to_world(depth):  # camera.hpp:42-48
        ndc = np.stack([2.0 * px / width - 1.0, -2.0 * py / height + 1.0, np.full(n, depth), np.ones(n)], axis=-1)
        world = ndc @ inverse_vp.T
        return world[:, :3] / world[:, 3:4]

    near, far = screen_to_world(0.0), screen_to_world(1.0)
    origin = near
    direction = far - near
    direction /= np.linalg.norm(direction, axis=-1, keepdims=True)  # vec3::direction(near, far) (:193)
    direction = rounded(direction, everyone)

    throughput = np.ones((n, 3))
    result = np.zeros((n, 3))
    bounced = np.zeros(n, dtype=bool)
    alive = everyone
    for _ in range(max_bounces):  # `if (!(max_bounces--)) return {}` (:157): a path that is still alive after the loop is black
        if alive.size == 0:
            break
        o, d = origin[alive], direction[alive]
        # test_planes (:36-60): the first plane at the smallest distance >= min_hit_dist
        best_plane_t = np.full(alive.size, np.inf)
        best_plane = np.full(alive.size, -1)
        for i in range(pod.n_planes):
            den = rounded(d @ plane_n[i], alive)
            with np.errstate(divide="ignore", invalid="ignore"):
                t = rounded(-(rounded(o @ plane_n[i], alive) + plane_d[i]) / den, alive)
            ok = (np.abs(den) > APPROX_ZERO) & (t >= 0.0) & (t >= MIN_HIT_DIST) & ~(t >= best_plane_t)  # `hit_dist <= *hit` keeps the earlier one
            best_plane_t = np.where(ok, t, best_plane_t)
            best_plane = np.where(ok, i, best_plane)
        # test_spheres (:62-87)
        best_sphere_t = np.full(alive.size, np.inf)
        best_sphere = np.full(alive.size, -1)
        for i in range(pod.n_spheres):
            e = centres[i] - o
            a = rounded(np.einsum("ij,ij->i", e, d), alive)
            e2 = rounded(np.einsum("ij,ij->i", e, e), alive)
            disc = radii[i] ** 2 - rounded(e2 - a * a, alive)
            f = rounded(np.sqrt(np.maximum(disc, 0.0)), alive)
            t = rounded(np.where(e2 < radii[i] ** 2, a + f, a - f), alive)  # from inside: the far root
            ok = (disc >= 0.0) & (t >= 0.0) & (t >= MIN_HIT_DIST) & ~(t >= best_sphere_t)
            best_sphere_t = np.where(ok, t, best_sphere_t)
            best_sphere = np.where(ok, i, best_sphere)
        # select(test_spheres, test_planes) (:96-102,160-161): the sphere unless the plane is strictly nearer
        sphere_wins = (best_sphere >= 0) & ((best_plane < 0) | (best_sphere_t <= best_plane_t))
        plane_wins = (best_plane >= 0) & ~sphere_wins
        hit = sphere_wins | plane_wins
        # miss: the sky (:163-164)
        missed = alive[~hit]
        t_sky = 0.5 * (direction[missed, 1] + 1.0)
        result[missed] = throughput[missed] * ((1.0 - t_sky)[:, None] * np.array([1.0, 1.0, 1.0]) + t_sky[:, None] * np.array([0.5, 0.7, 1.0]))
        # hit: position, normal, material
        lanes = alive[hit]
        if lanes.size == 0:
            alive = lanes
            break
        bounced[lanes] = True
        distance = np.where(sphere_wins, best_sphere_t, best_plane_t)[hit]
        position = rounded(origin[lanes] + direction[lanes] * distance[:, None], lanes)  # r.at(hit.distance)
        is_sphere = sphere_wins[hit]
        sphere_index = np.maximum(best_sphere[hit], 0)
        plane_index = np.maximum(best_plane[hit], 0)
        outward = position - (centres[sphere_index] if pod.n_spheres else np.zeros((lanes.size, 3)))
        outward /= np.maximum(np.linalg.norm(outward, axis=-1, keepdims=True), 1e-300)  # vec3::direction(center, r.at(t)) (:85)
        outward = rounded(outward, lanes)
        normal = np.where(is_sphere[:, None], outward, plane_n[plane_index] if pod.n_planes else outward)
        material = np.where(is_sphere, sphere_material[sphere_index] if pod.n_spheres else 0, plane_material[plane_index] if pod.n_planes else 0)
        # which scatter function (mg: :142-152 — metal, everything else lambert; sm: sm_ray_tracer.cpp:221-236 — dielectric, air,
        # vacuum, water and ice refract as well)
        metal = kind[material] == METAL
        refracts = np.isin(kind[material], REFRACTING) if sm_materials else np.zeros(lanes.size, dtype=bool)
        diffuse = ~refracts
        unit = np.zeros((lanes.size, 3))
        unit[diffuse] = streams.unit_vector(lanes[diffuse])  # lambert and metal draw a unit vector, dielectric_scatter ONE number
        unit = rounded(unit, lanes) * unit_scale[lanes][:, None]
        # lambert_scatter (:110-123)
        lambert = rounded(normal + unit, lanes)
        tiny = np.all(np.abs(lambert) <= APPROX_ZERO, axis=-1)
        lambert = np.where(tiny[:, None], normal, lambert)
        # metal_scatter (:126-140); reflect(v, n) = v - 2 dot(v, n) n (src/common.hpp:100-103)
        incoming = direction[lanes]
        v = incoming / np.linalg.norm(incoming, axis=-1, keepdims=True)
        reflected = v - 2.0 * np.einsum("ij,ij->i", v, normal)[:, None] * normal
        shiny = reflected + roughness[material][:, None] * unit
        absorbed = metal & (rounded(np.einsum("ij,ij->i", shiny, normal), lanes) <= 0.0)  # `return {}`: the sample is black
        scatter = np.where(metal[:, None], shiny, lambert)
        scatter /= np.maximum(np.linalg.norm(scatter, axis=-1, keepdims=True), 1e-300)
        scatter = rounded(scatter, lanes)
        if refracts.any():
            # dielectric_scatter, sm_ray_tracer.cpp:156-219, as written: the incoming direction is NOT normalised, nor is the new one
            index_of_refraction = reflectivity[material]
            d_n = np.einsum("ij,ij->i", incoming, normal)
            from_inside = d_n > 0.0
            outward_normal = np.where(from_inside[:, None], -normal, normal)
            eta = np.where(from_inside, index_of_refraction, 1.0 / index_of_refraction)
            length = np.linalg.norm(incoming, axis=-1)
            cosine = np.where(from_inside, index_of_refraction * d_n / length, -d_n / length)
            mirrored = incoming - 2.0 * d_n[:, None] * normal  # reflect(r.direction, hit.normal) (:188)
            cos_i = -np.einsum("ij,ij->i", incoming, outward_normal)  # refract (:161-172)
            sin2_t = eta * eta * (1.0 - cos_i * cos_i)
            can_refract = ~(sin2_t > 1.0)
            cos_t = np.sqrt(np.maximum(1.0 - sin2_t, 0.0))
            refracted = eta[:, None] * incoming + (eta * cos_i - cos_t)[:, None] * outward_normal
            r0 = ((1.0 - index_of_refraction) / (1.0 + index_of_refraction)) ** 2  # schlick (:174-179)
            reflect_probability = np.where(can_refract, r0 + (1.0 - r0) * (1.0 - cosine) ** 5, 1.0)
            u = np.zeros(lanes.size)
            u[refracts] = streams.next(lanes[refracts])
            through = np.where((u < reflect_probability)[:, None], mirrored, refracted)
            scatter = np.where(refracts[:, None], through, scatter)
        throughput[lanes] = throughput[lanes] * attenuation_of[material]
        origin[lanes] = position
        direction[lanes] = scatter
        alive = lanes[~absorbed]
    # `colour /= samples_per_pixel` (:195)
    return result.reshape(n_runs, height, width, spp, 3).mean(axis=3), bounced.reshape(n_runs, height, width, spp).any(axis=3)


def render_f64(pod, width, height, seed, sm_materials=False):
    """float64 mean colour per pixel, [height, width, 3]: no run perturbed"""
    return trace(pod, width, height, seed, sm_materials)[0][0]


@dataclasses.dataclass(frozen=True)
class Allowance:
    base: np.ndarray  # [h, w, 3] float64: the unperturbed mean
    scale: np.ndarray  # [h, w]: max(|base| over channels, SCALE_FLOOR)
    spread: np.ndarray  # [h, w]: the largest |run - base| of the ensemble, any channel
    allowance: np.ndarray  # [h, w]: ROUNDING * scale + SPREAD_FACTOR * spread
    tight: np.ndarray  # [h, w] bool: allowance <= TIGHT * scale
    bounced: np.ndarray  # [h, w] bool: a sample of the pixel hits something (in the unperturbed run)

    def excess(self, frame):
        """|frame - base| / allowance per pixel (largest channel): at most 1 inside the rule"""
        return np.abs(np.asarray(frame, dtype=np.float64) - self.base).max(axis=-1) / self.allowance


def allowance_of(pod, width, height, seed, amplitude, runs, noise_seed):
    """The per-pixel rule for one frame from an ensemble of `runs` runs at `amplitude` ulps.  Arrays are read-only: share them."""
    frames, bounced = trace(pod, width, height, seed, runs=[EXACT] + [Run(amplitude=amplitude)] * runs, noise_seed=noise_seed)
    base = frames[0]
    spread = np.abs(frames[1:] - base).max(axis=(0, -1))
    scale = np.maximum(np.abs(base).max(axis=-1), SCALE_FLOOR)
    allowance = ROUNDING * scale + SPREAD_FACTOR * spread
    out = Allowance(base, scale, spread, allowance, allowance <= TIGHT * scale, bounced[0])
    for array in dataclasses.astuple(out):
        array.setflags(write=False)
    return out


def pack(mean):
    """RGBA8 colour channels of a mean, [..., 3] ints: clamp01(sqrt(c)) * 255.99999 truncated, as the worker packs (oracle/cpu_ref.cpp pack)."""
    return (np.clip(np.sqrt(np.maximum(np.asarray(mean, dtype=np.float64), 0.0)), 0.0, 1.0) * 255.99999).astype(np.int64)


def channels(rgba):
    """uint32 RGBA8888 -> its three colour channels, [..., 3] ints"""
    return np.stack([(rgba >> s) & 255 for s in (24, 16, 8)], axis=-1).astype(np.int64)
