// rt_amd/csrc/bvh_scan.hpp — RT_HIP_FLAG_BVH: the sphere query through the hierarchy of bvh.hpp, per lane.  Shared by the
// render kernel (kernels.hip, render_queue<-4>) and the known-answer kernel of the test-only library (kat.hip).
//
// SAME ANSWER AS THE LINEAR SCAN.  test_spheres keeps the lexicographic minimum of (t, index) over the spheres it accepts
// (scan.hpp, and scan_spheres_together in scan_streamed.hpp).  The traversal below
//   * tests every sphere it reaches with probe_sphere and the square-root half of finish_sphere, on the same (c, r^2) floats;
//   * accepts a candidate when t < best.t || (t == best.t && index < best.index), `index` being the sphere's scene index;
//   * culls a box only where no sphere inside can produce a computed t that would be accepted (the bound below).
// So it returns the linear scan's sphere, bit for bit, whatever order it meets them in.  The one thing a minimum cannot
// reproduce is a NaN distance, which the sequential rule lets in and then never displaces consistently; a lane that meets a
// non-finite t, or whose ray is degenerate, is reported and its caller runs the linear scan for it instead.
//
// THE CULL BOUND.  u = 2^-24.  A sphere (c, r2) of the tree, a ray (o, d) with |d|^2 = 1 + k, |k| <= 2^-21 + 2^-22 (the test on the
// computed dot(d, d) below admits 1 -/+ 2^-21), e = c - o, U = |e| + sqrt(r2).  The probe computes e, a = e.d, e2 = e.e with
// relative errors of at most u, 3u|e||d| and 4u|e|^2, disc = r2 - fma(-a, a, e2), f = sqrt(disc), t = a -/+ f, each rounded once.
// With h^2 = |e|^2 - (e.d)^2, the point P = o + t d the computed t stands for satisfies
//   |P - c|^2 = (t - e.d)^2 + h^2 + t^2 k <= r2 + 32 u U^2 + 4.1 |k| U^2 <= r2 + 81 u U^2 < r2 + 2^-17.3 U^2
// (|a - e.d| <= 4u|e|, |e2 - a^2 - h^2| <= 14u|e|^2 before the fma's and the subtraction's roundings, |t| <= 2.01 U, |f| <= 1.01 U),
// so every computed hit lies within delta = sqrt(r2 + 2^-17.3 U^2) - sqrt(r2) < 2^-8.65 U of the sphere, hence of its box.  The
// builder's ball (C, R) holds every tree sphere: |c - C| + sqrt(r2) <= R, so U <= |o - C| + R.  Per query the margin is
//   pad = 2^-8 (|o - C| + R) + 2^-64      (the second term covers products that underflow: their absolute errors are 2^-149)
// and a node is entered when the ray meets its box grown by `pad` somewhere in [-pad, best.t + pad].  The box grown by pad holds
// P with pad - delta > 2^-9.9 (|o - C| + R) to spare; the slab arithmetic ((lo - o) - pad, times a rounded 1 / d) errs by at
// most 5u (|o - C| + R + pad) on either side of a t that can be accepted — far inside that spare.  A sphere whose t could win
// has t <= best.t, and fl(best.t + pad) >= best.t + 5uU wherever that matters (best.t <= 2.5 U; beyond, no tree sphere's t
// comes near best.t anyway).  The adversarial rays of tests/test_gpu_bvh.py (tangents at +-1..64 ulp, origins on and inside
// spheres, duplicates) and the RT_HIP_BVH_CHECK build over config 5's 300 M queries check it at one scale.  Across the scales
// the builder admits (2^-60 .. 2^38, r^2 down to subnormal and zero), origins up to 1e6 scene widths away, scenes 1e6 widths
// off the coordinate origin, and directions with zero, subnormal and tiny components from origins on box faces,
// tests/test_bvh_cull_audit.py audits on the host that no box between the root and the oracle's answer is culled (with a pad
// no larger than the one computed here), and test_closest_hit_in_every_regime_of_the_cull_bound of tests/test_gpu_bvh.py runs
// the same scenes and rays through this code; test_directions_at_the_edges_of_the_length_gate sits on both sides of the
// |d|^2 gate, test_a_ray_that_fills_the_stack and test_frames_of_a_tree_as_deep_as_the_stack use the last stack word, and
// test_frames_whose_lanes_fall_back_to_the_linear_scan runs the render kernel's rescan.  Measured there, the margin has a factor
// of 4 to 16 to spare, not more: the audit still passes at 2^-10 and fails at 2^-12 (profiles/r07/README.md).
#pragma once

#include "bvh.hpp"
#include "scan.hpp"

namespace rt_hip
{
	// one sphere for this lane alone: the arithmetic of probe_sphere / finish_sphere, the (t, index) rule of a minimum
	__device__ __forceinline__ void offer_sphere(candidate& best, bool& bad, vec3 o, vec3 d, float4 s, uint32_t index)
	{
		const sphere_probe p = probe_sphere(o, d, s);
		if (p.pos)
		{
			const float f = sqrt_rn(p.disc);
			const float t = (p.e2 < s.w) ? p.a + f : p.a - f;
			bad = bad || !(__builtin_fabsf(t) <= 3.402823466e38f); // NaN or infinite: the sequential rule is order-dependent there
			const bool accept = !(t < min_hit_dist) && (!best.have || t < best.t || (t == best.t && index < best.index));
			best.t = accept ? t : best.t;
			best.index = accept ? index : best.index;
			best.have = best.have || accept;
		}
	}

	// does the ray meet box [lo, hi] grown by pad within [-pad, bound]?  `near` = where it enters (for the visiting order)
	__device__ __forceinline__ bool enter_box(float4 lo, float4 hi, vec3 o, vec3 inv, float pad, float bound, float& near)
	{
		const float x0 = ((lo.x - o.x) - pad) * inv.x, x1 = ((hi.x - o.x) + pad) * inv.x;
		const float y0 = ((lo.y - o.y) - pad) * inv.y, y1 = ((hi.y - o.y) + pad) * inv.y;
		const float z0 = ((lo.z - o.z) - pad) * inv.z, z1 = ((hi.z - o.z) + pad) * inv.z;
		// (fminf / fmaxf drop a NaN — 0 * inf where the ray runs in a slab's plane — which only ever widens the interval)
		const float t_near = fmaxf(fmaxf(fminf(x0, x1), fminf(y0, y1)), fminf(z0, z1));
		const float t_far = fminf(fminf(fmaxf(x0, x1), fmaxf(y0, y1)), fmaxf(z0, z1));
		near = t_near;
		return t_near <= t_far + pad && t_near <= bound && t_far >= -pad;
	}

	// The spheres' closest hit for this lane: the always list, then the tree.  `stack` = this lane's first word of its LDS stack
	// (entries block_threads words apart, bvh_max_depth of them).  False: the lane's answer must come from the linear scan.
	__device__ __forceinline__ bool bvh_spheres(candidate& best, vec3 o, vec3 d, const device_bvh& b, const float4* __restrict__ geometry, uint32_t* stack)
	{
		bool bad = false;
		for (uint32_t k = 0; k < b.n_always; k++) // (wave-uniform: scalar loads)
		{
			const uint32_t i = b.always[k];
			offer_sphere(best, bad, o, d, geometry[i], i);
		}
		if (b.n_tree == 0)
			return !bad;
		const vec3 oc = { o.x - b.cx, o.y - b.cy, o.z - b.cz };
		const float pad = (sqrt_rn(dot(oc, oc)) + b.radius) * 0x1p-8f + 0x1p-64f;
		const float dd = dot(d, d);
		// a finite origin gives a finite pad; |d|^2 within 2^-21 of 1 also says d is finite
		if (!(pad <= 0x1p100f && dd >= 1.0f - 0x1p-21f && dd <= 1.0f + 0x1p-21f))
			return false;
		const vec3 inv = { 1.0f / d.x, 1.0f / d.y, 1.0f / d.z };
		uint32_t link = b.root, depth = 0;
		while (true)
		{
			if (link & bvh_leaf_bit)
			{
				const uint32_t first = link & ((1u << 29) - 1u), count = ((link >> 29) & 3u) + 1u;
				for (uint32_t j = 0; j < count; j++)
					offer_sphere(best, bad, o, d, b.spheres[first + j], b.order[first + j]);
			}
			else
			{
				const float4* const node = b.nodes + static_cast<size_t>(link) * 4u;
				const float4 a_lo = node[0], a_hi = node[1], b_lo = node[2], b_hi = node[3];
				const float bound = best.have ? best.t + pad : __builtin_inff();
				float near_a, near_b;
				const bool in_a = enter_box(a_lo, a_hi, o, inv, pad, bound, near_a);
				const bool in_b = enter_box(b_lo, b_hi, o, inv, pad, bound, near_b);
				const uint32_t link_a = __float_as_uint(a_lo.w), link_b = __float_as_uint(a_hi.w);
				if (in_a && in_b)
				{
					// the nearer child first; the other waits on the stack (depth <= bvh_max_depth by construction: the
					// guard only keeps a corrupt tree from writing past the lane's stack)
					if (depth >= bvh_max_depth)
						return false;
					const bool a_first = near_a <= near_b;
					stack[depth * block_threads] = a_first ? link_b : link_a;
					depth++;
					link = a_first ? link_a : link_b;
					continue;
				}
				if (in_a || in_b)
				{
					link = in_a ? link_a : link_b;
					continue;
				}
			}
			if (depth == 0)
				break;
			depth--;
			link = stack[depth * block_threads];
		}
		return !bad;
	}
}
