// rt_amd/csrc/box_bvh_scan.hpp — RT_HIP_FLAG_BOX_BVH: the box query through the hierarchy of box_bvh.hpp, per lane.  Shared by the
// render kernel (kernels.hip, render_queue<scan_bvh_boxtree>) and the known-answer kernel of the test-only library (kat.hip).
//
// SAME ANSWER AS THE LINEAR SCAN.  test_box (scan.hpp) decides every box by itself — hits_box_given's t, accepted when
// !(t < min_hit_dist) — and scan_boxes keeps the first of the smallest: the lexicographic minimum of (t, index) over the boxes it
// accepts.  (An accepted t is never a NaN: a hit asks tmax >= tmin and t is one of the two.)  The traversal below
//   * tests every box it reaches with hits_box_given on the same two float4s (leaf-ordered bit copies) and the same
//     box_reciprocals(d);
//   * accepts a candidate when !(t < min_hit_dist) and t < best.t || (t == best.t && index < best.index), `index` being the box's
//     scene index;
//   * skips a node only where no box inside it can produce an accepted t that would win (the cull below).
// So it returns the linear scan's box, bit for bit, whatever order it meets them in.
//
// THE CULL rests on monotone rounding and needs no pad.  A tree box has finite corners, and its extent lo_b <= hi_b per axis (the
// min and max of its two corners: hits_box_given's selects make a box with lo > hi the swapped box) lies within every node N above
// it EXACTLY: lo_N <= lo_b, hi_b <= hi_N (box_bvh.cpp: unions by min and max, which do not round).  The node test computes
// fl((lo_N - o) inv) and fl((hi_N - o) inv) with the operations hits_box_given applies to the box, in the same order, on the same o
// and inv.  For NaN-free operands a rounded subtraction is monotone in its first operand and a rounded product with a fixed factor
// is monotone (increasing for inv > 0, decreasing for inv < 0; overflow to an infinity keeps the order).  Per axis, with inv > 0:
//   near_N = fl(fl(lo_N - o) inv) <= fl(fl(lo_b - o) inv) = near_b,   far_N = fl(fl(hi_N - o) inv) >= fl(fl(hi_b - o) inv) = far_b,
// and with inv < 0 the same with lo and hi exchanged; select_min / select_max pick near and far out of the two products on both sides
// (no NaN: they are the true minimum and maximum).  The maximum of three and the minimum of three are monotone too:
//   tmin_N <= tmin_b   and   tmax_N >= tmax_b.
// A box that hits has tmax_b >= tmin_b and tmax_b >= 0, and its t is tmin_b or tmax_b, so t >= tmin_b >= tmin_N; hence
// tmax_N >= tmax_b >= tmin_b >= tmin_N and tmax_N >= 0.  A node may therefore be skipped exactly when
//   !(tmax_N >= tmin_N) || tmax_N < 0 || tmin_N > best.t
// (t == best.t may still win by its index: the last comparison is strict).  enter_node writes the complement with every comparison
// the other way round, so that a NaN — which the gate below keeps out — would ENTER a node and never cull one.
//
// THE GATE.  The argument needs NaN-free operands: 0 x inf is the one way hits_box_given makes a NaN from finite corners, and it
// takes an infinite reciprocal (a zero or subnormal direction component: the grazing case of DESIGN.md §3.7, whose answer depends on
// which operand of a select the NaN is), a zero reciprocal (an infinite component) meeting a difference that overflowed, or a
// non-finite origin or direction.  A lane whose three reciprocals are not all finite and non-zero, or whose origin is not finite,
// is reported and its caller scans device_scene::box_bounds linearly instead, as bvh_spheres sends its degenerate lanes to the
// linear scan.  (Zero components are not treated more cheaply: a ray inside a slab it runs along would need the slab's test at
// every node, and such lanes are rare — an axis-parallel camera ray at most.)  Boxes with a non-finite corner are not in the tree:
// the builder's ALWAYS list, tested by every query with the same arithmetic.
// tests/test_box_bvh_cull_audit.py restates the node test in binary32 on the host and audits, across scales 2^-60 .. 2^38, origins
// on faces and edges, inside nested boxes and far away, and tiny, subnormal and overflowing components, that no node between the
// root and the restatement's answer is skipped; tests/test_gpu_box_bvh.py runs this code against tests/native/box_reference.cpp.
#pragma once

#include "box_bvh.hpp"
#include "scan.hpp"

namespace rt_hip
{
	// The box hierarchy's descriptor in device memory.  It lies box_bvh_descriptor_offset bytes behind the sphere hierarchy's
	// (device_bvh), which the hierarchy kernel is handed in the item_sums argument's place: no kernel's argument block changes.
	struct device_box_bvh
	{
		const float4* nodes;	// 4 per inner node
		const float4* corners;	// 2 per tree box in leaf order: bit copies of its pair in device_scene::box_bounds
		const uint32_t* order;	// their indices in the scene
		const uint32_t* always; // indices of the boxes outside the tree (tested by every query)
		uint32_t root, n_tree, n_always, reserved;
	};
	constexpr size_t box_bvh_descriptor_offset = 64;
	static_assert(sizeof(device_bvh) <= box_bvh_descriptor_offset, "the box hierarchy's descriptor lies behind the sphere hierarchy's");

	// one box for this lane alone: test_box's arithmetic, the (t, index) rule of a minimum
	__device__ __forceinline__ void offer_box(candidate& best, vec3 o, vec3 inv, float4 lo, float4 hi, uint32_t index)
	{
		float t = 0.0f;
		const bool hit = hits_box_given(o, inv, { lo.x, lo.y, lo.z }, { hi.x, hi.y, hi.z }, t);
		const bool accept = hit && !(t < min_hit_dist) && (!best.have || t < best.t || (t == best.t && index < best.index));
		best.t = accept ? t : best.t;
		best.index = accept ? index : best.index;
		best.have = best.have || accept;
	}

	// may a box within the node box [lo, hi] still win?  hits_box_given's own operations on the node's corners (the cull above);
	// `near` = tmin_N, for the visiting order
	__device__ __forceinline__ bool enter_node(float4 lo, float4 hi, vec3 o, vec3 inv, const candidate& best, float& near)
	{
		const vec3 t1 = (vec3{ lo.x, lo.y, lo.z } - o) * inv;
		const vec3 t2 = (vec3{ hi.x, hi.y, hi.z } - o) * inv;
		const float tmin = select_max(select_max(select_min(t1.x, t2.x), select_min(t1.y, t2.y)), select_min(t1.z, t2.z));
		const float tmax = select_min(select_min(select_max(t1.x, t2.x), select_max(t1.y, t2.y)), select_max(t1.z, t2.z));
		near = tmin;
		return !(tmax < tmin) && !(tmax < 0.0f) && !(best.have && tmin > best.t);
	}

	// the gate: every reciprocal finite and not zero, the origin finite (a NaN fails every comparison)
	__device__ __forceinline__ bool box_bvh_takes(vec3 o, vec3 inv)
	{
		constexpr float largest = 3.402823466e38f;
		const float ix = __builtin_fabsf(inv.x), iy = __builtin_fabsf(inv.y), iz = __builtin_fabsf(inv.z);
		const bool reciprocals = ix <= largest && iy <= largest && iz <= largest && ix > 0.0f && iy > 0.0f && iz > 0.0f;
		return reciprocals && __builtin_fabsf(o.x) <= largest && __builtin_fabsf(o.y) <= largest && __builtin_fabsf(o.z) <= largest;
	}

	// The boxes' closest hit for this lane: the always list, then the tree.  `inv` = box_reciprocals(d); `bounds` = the scene's pairs
	// (device_scene::box_bounds); `stack` = this lane's first word of its LDS stack (entries block_threads words apart, bvh_max_depth
	// of them: the sphere traversal has finished with it).  False: the lane's answer must come from the linear scan, `best` is void.
	__device__ __forceinline__ bool bvh_boxes(candidate& best, vec3 o, vec3 inv, const device_box_bvh& b, const float4* __restrict__ bounds, uint32_t* stack)
	{
		if (!box_bvh_takes(o, inv))
			return false;
		for (uint32_t k = 0; k < b.n_always; k++) // (wave-uniform: scalar loads)
		{
			const uint32_t i = b.always[k];
			offer_box(best, o, inv, bounds[2u * i], bounds[2u * i + 1u], i);
		}
		if (b.n_tree == 0)
			return true;
		uint32_t link = b.root, depth = 0;
		while (true)
		{
			if (link & bvh_leaf_bit)
			{
				const uint32_t first = link & ((1u << 29) - 1u), count = ((link >> 29) & 3u) + 1u;
				for (uint32_t j = 0; j < count; j++)
					offer_box(best, o, inv, b.corners[2u * (first + j)], b.corners[2u * (first + j) + 1u], b.order[first + j]);
			}
			else
			{
				const float4* const node = b.nodes + static_cast<size_t>(link) * 4u;
				const float4 a_lo = node[0], a_hi = node[1], b_lo = node[2], b_hi = node[3];
				float near_a, near_b;
				const bool in_a = enter_node(a_lo, a_hi, o, inv, best, near_a);
				const bool in_b = enter_node(b_lo, b_hi, o, inv, best, near_b);
				const uint32_t link_a = __float_as_uint(a_lo.w), link_b = __float_as_uint(a_hi.w);
				if (in_a && in_b)
				{
					// the nearer child first; the other waits on the stack (depth <= bvh_max_depth by construction: the guard only
					// keeps a corrupt tree from writing past the lane's stack)
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
		return true;
	}
}
