// rt_amd/csrc/scan_streamed.hpp — the sphere scans that read the (center, radius^2) table in memory instead of a copy in LDS
// (next to scan.hpp, whose probe_sphere / finish_sphere they are made of):
//   * scan_streamed_spheres: wave-uniform scalar loads, the next group's load issued before this group's probes.  Used by the
//     streamed kernels (scan_streamed, scan_streamed_dense), the resident kernel's scalar-load build (scan_resident, NP == 1) and the
//     hierarchy kernel's fall-back for the lanes its traversal does not take (scan_bvh and its pass / box / light builds);
//   * scan_spheres_together: the cooperative scan of a wave that holds a handful of rays.  Used by scan_streamed alone.
#pragma once

#include "scan.hpp"

namespace rt_hip
{
	// The streamed kernel's sphere scan: the (center, radius^2) table is read from HBM/L2 with wave-uniform scalar loads,
	// four spheres = 64 bytes = one s_load_dwordx16.  Every wave of a CU walks the 1.6 MB table at its own position, so
	// the 16 KB scalar cache holds next to nothing of it (SQC_DCACHE: 29 % hits at 100 000 spheres,
	// profiles/r03/config5_streamed/) and most loads come from L2.  The load of group g+1 is therefore issued BEFORE
	// group g is probed (two register sets, the loop unrolled by two so that no set is ever copied): the wave has 48
	// vector instructions to issue while its next 64 bytes are on their way.
	__device__ __forceinline__ void probe_group(candidate& best, vec3 o, vec3 d, float4 s0, float4 s1, float4 s2, float4 s3, uint32_t first_index)
	{
		const sphere_probe p0 = probe_sphere(o, d, s0);
		const sphere_probe p1 = probe_sphere(o, d, s1);
		const sphere_probe p2 = probe_sphere(o, d, s2);
		const sphere_probe p3 = probe_sphere(o, d, s3);
		const unsigned long long m0 = __builtin_amdgcn_ballot_w64(p0.pos), m1 = __builtin_amdgcn_ballot_w64(p1.pos);
		const unsigned long long m2 = __builtin_amdgcn_ballot_w64(p2.pos), m3 = __builtin_amdgcn_ballot_w64(p3.pos);
		if ((m0 | m1 | m2 | m3) != 0)
		{
			finish_sphere(best, p0, s0.w, first_index, m0);
			finish_sphere(best, p1, s1.w, first_index + 1, m1);
			finish_sphere(best, p2, s2.w, first_index + 2, m2);
			finish_sphere(best, p3, s3.w, first_index + 3, m3);
		}
	}

	__device__ __forceinline__ void scan_streamed_spheres(candidate& best, vec3 o, vec3 d, const float4* __restrict__ table, uint32_t count)
	{
		const uint32_t groups = count >> 2;
		if (groups)
		{
			float4 a0 = table[0], a1 = table[1], a2 = table[2], a3 = table[3];
			uint32_t g = 0;
			for (; g + 2 <= groups; g += 2)
			{
				const float4* const b = table + (g + 1) * 4;
				const float4 b0 = b[0], b1 = b[1], b2 = b[2], b3 = b[3];
				probe_group(best, o, d, a0, a1, a2, a3, g * 4);
				const float4* const a = table + (g + 2 < groups ? g + 2 : groups - 1) * 4; // (past the end: the last group again, unused)
				a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3];
				probe_group(best, o, d, b0, b1, b2, b3, (g + 1) * 4);
			}
			if (g < groups)
				probe_group(best, o, d, a0, a1, a2, a3, g * 4);
		}
		for (uint32_t i = groups * 4; i < count; i++)
			test_sphere(best, o, d, table[i], i);
	}

	// SPARSE WAVES (streamed kernel).  A scan costs a wave the same whether one lane holds a ray or all 64 do.  At the
	// end of a launch — and in small frames of big scenes — waves hold a handful of rays: such a wave turns the scan
	// around and walks the table ONCE PER RAY with all 64 lanes, lane l testing spheres l, l + 64, ... (coalesced 16-byte
	// loads), followed by a wave-wide minimum.  test_spheres keeps the first sphere at the smallest accepted distance
	// (`hit_dist <= *hit` -> continue, mg_ray_tracer.cpp:74), i.e. the lexicographic minimum of (t, index) over the
	// accepted candidates; every lane takes that minimum over its own spheres in index order, and the 64 partial results
	// are reduced with the same order — accepted distances are >= 0.001, so their bit patterns order like the numbers.
	// The one thing a minimum cannot reproduce is a NaN distance (a degenerate ray), which the sequential rule lets
	// in and then never displaces consistently: if any lane meets one, the ray is reported as not scanned and goes
	// through the sequential scan.  The per-sphere arithmetic is finish_sphere's, bit for bit.
	constexpr uint32_t sparse_min_spheres = sparse_launch_min_spheres; // (below that a sequential scan is a few microseconds anyway)

	__device__ __forceinline__ void test_sphere_alone(candidate& best, bool& met_nan, vec3 o, vec3 d, float4 s, uint32_t index)
	{
		const sphere_probe p = probe_sphere(o, d, s);
		if (p.pos) // a per-lane branch: every lane looks at a different sphere, and few spheres lie on a ray's line
		{
			const float f = sqrt_rn(p.disc);
			const float t = (p.e2 < s.w) ? p.a + f : p.a - f;
			met_nan = met_nan || t != t;
			const bool accept = !(t < min_hit_dist) && !(best.have && best.t <= t);
			best.t = accept ? t : best.t;
			best.index = accept ? index : best.index;
			best.have = best.have || accept;
		}
	}

	// call converged, with a wave-uniform ray; returns false if the ray has to be scanned sequentially instead
	__device__ __forceinline__ bool scan_spheres_together(candidate& found, vec3 o, vec3 d, const float4* __restrict__ table, uint32_t count, uint32_t lane)
	{
		candidate mine = { 0.0f, 0u, false };
		bool met_nan = false;
		uint32_t i = lane;
		// four independent loads in flight per lane: the walk is bound by L2 latency, not by arithmetic.  (The registers
		// they take cost the kernel one wave per SIMD of occupancy, 5 instead of 6, which the sequential scan — bound by
		// vector issue — does not miss: config 5 5.61 against 5.69 s with two loads in flight, 10 000 spheres 277 against
		// 290 ms; profiles/r03/config5_streamed/sparse_waves_ab.txt.)
		for (; i + 192u < count; i += 256u)
		{
			const float4 s0 = table[i], s1 = table[i + 64u], s2 = table[i + 128u], s3 = table[i + 192u];
			test_sphere_alone(mine, met_nan, o, d, s0, i);
			test_sphere_alone(mine, met_nan, o, d, s1, i + 64u);
			test_sphere_alone(mine, met_nan, o, d, s2, i + 128u);
			test_sphere_alone(mine, met_nan, o, d, s3, i + 192u);
		}
		for (; i < count; i += 64u)
			test_sphere_alone(mine, met_nan, o, d, table[i], i);
		if (__builtin_amdgcn_ballot_w64(met_nan) != 0)
			return false;
		uint32_t key_t = mine.have ? __float_as_uint(mine.t) : 0xFFFFFFFFu; // (no accepted distance has this pattern: it is a NaN's)
		uint32_t key_i = mine.have ? mine.index : 0xFFFFFFFFu;
#pragma unroll
		for (int offset = 32; offset > 0; offset >>= 1)
		{
			const uint32_t other_t = __shfl_xor(key_t, offset, 64);
			const uint32_t other_i = __shfl_xor(key_i, offset, 64);
			const bool take = other_t < key_t || (other_t == key_t && other_i < key_i);
			key_t = take ? other_t : key_t;
			key_i = take ? other_i : key_i;
		}
		found.have = key_t != 0xFFFFFFFFu;
		found.t = found.have ? __uint_as_float(key_t) : 0.0f;
		found.index = found.have ? key_i : 0u;
		return true;
	}
}
