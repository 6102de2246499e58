// rt_amd/csrc/bvh_build.hpp — the per-element steps of the device builder of the sphere hierarchy (RT_HIP_FLAG_BVH_DEVICE_BUILD,
// bvh_build.hip), written so that g++ compiles them too: tests/native/lbvh_reference.cpp restates the whole build serially over
// these very functions, and the device tree must equal that restatement byte for byte.
//
// The tree is the layout of bvh.hpp.  What differs from the host builder (bvh.cpp) is the topology only: the tree spheres are
// ordered by (30-bit Morton code of the centre, scene index) and a range is cut at the highest differing bit of that key, or at
// its middle where that cut would leave a half too large for the levels left.  Which spheres stay out of the tree, the
// per-sphere boxes and the ball are the host builder's, rule for rule.
//
// Leaf slot k is position k of the sorted order, and the inner node that cuts the sorted order between positions p - 1 and p is
// node p - 1: every cut position belongs to at most one node, so the numbering needs no prefix sum and depends on nothing but
// the keys.  Node slots that no cut uses stay zero and nothing links to them.
//
// Every float comparison that decides a byte goes through `ordered`, a total order on binary32 (-0 below +0): minima and maxima
// are then associative and commutative bit for bit, whatever order a reduction takes them in.  The binary64 steps are single
// correctly rounded operations (subtract, add, divide, multiply, square root): both compilers are told not to contract them.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define RT_HIP_LBVH_FN __host__ __device__ inline
#else
#define RT_HIP_LBVH_FN inline
#endif

namespace rt_hip
{
namespace lbvh
{
	constexpr uint32_t max_depth = 24;			   // bvh_max_depth
	constexpr uint32_t leaf_spheres = 4;		   // bvh_leaf_spheres
	constexpr uint32_t leaf_bit = 1u << 31;		   // bvh_leaf_bit
	constexpr uint32_t max_spheres = 1u << 26;	   // bvh_max_tree_spheres: what the builder takes at all (it learns the tree's share on the device only)
	constexpr uint32_t not_in_tree = 0xFFFFFFFFu; // sort key of a sphere outside the tree: behind every Morton code

	RT_HIP_LBVH_FN uint32_t bits_of(float f) { return __builtin_bit_cast(uint32_t, f); }
	RT_HIP_LBVH_FN float float_of(uint32_t u) { return __builtin_bit_cast(float, u); }

	// a total order on binary32 as unsigned integers: negative values reversed below the positive ones
	RT_HIP_LBVH_FN uint32_t ordered(float f)
	{
		const uint32_t u = bits_of(f);
		return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
	}
	RT_HIP_LBVH_FN float unordered(uint32_t o) { return float_of((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o); }
	RT_HIP_LBVH_FN float min_of(float a, float b) { return ordered(b) < ordered(a) ? b : a; }
	RT_HIP_LBVH_FN float max_of(float a, float b) { return ordered(b) > ordered(a) ? b : a; }

	// the neighbours of a finite binary32 (nextafter towards -inf / +inf)
	RT_HIP_LBVH_FN float next_down(float f)
	{
		const uint32_t u = bits_of(f);
		if ((u & 0x7FFFFFFFu) == 0u)
			return float_of(0x80000001u);
		return float_of((u & 0x80000000u) ? u + 1u : u - 1u);
	}
	RT_HIP_LBVH_FN float next_up(float f)
	{
		const uint32_t u = bits_of(f);
		if ((u & 0x7FFFFFFFu) == 0u)
			return float_of(0x00000001u);
		return float_of((u & 0x80000000u) ? u - 1u : u + 1u);
	}
	// binary32 at or below / at or above a binary64 value (bvh.cpp, down / up)
	RT_HIP_LBVH_FN float down(double v)
	{
		float f = static_cast<float>(v);
		if (static_cast<double>(f) > v)
			f = next_down(f);
		return f;
	}
	RT_HIP_LBVH_FN float up(double v)
	{
		float f = static_cast<float>(v);
		if (static_cast<double>(f) < v)
			f = next_up(f);
		return f;
	}

	// which spheres the tree can take (bvh.cpp:201-203): 0 <= r^2 <= 2^80 and |c| <= 2^40; a NaN fails
	RT_HIP_LBVH_FN bool tame(const float g[4])
	{
		bool t = g[3] >= 0.0f && g[3] <= 0x1p80f;
		for (int j = 0; j < 3; j++)
			t = t && __builtin_fabsf(g[j]) <= 0x1p40f;
		return t;
	}
	RT_HIP_LBVH_FN double half_width(float r2) { return __builtin_sqrt(static_cast<double>(r2)); }
	RT_HIP_LBVH_FN void sphere_box(const float g[4], float lo[3], float hi[3])
	{
		const double half = half_width(g[3]);
		for (int j = 0; j < 3; j++)
		{
			lo[j] = down(static_cast<double>(g[j]) - half);
			hi[j] = up(static_cast<double>(g[j]) + half);
		}
	}
	// widest extent of the tame centres (bvh.cpp:221-224)
	RT_HIP_LBVH_FN double extent_of(const float cmin[3], const float cmax[3])
	{
		double extent = 0.0;
		for (int j = 0; j < 3; j++)
		{
			const double lo = cmin[j], hi = cmax[j];
			if (hi > lo && hi - lo > extent)
				extent = hi - lo;
		}
		return extent;
	}
	RT_HIP_LBVH_FN bool large(float r2, double extent) { return half_width(r2) > extent / 4.0; }
	RT_HIP_LBVH_FN uint32_t large_cap(uint32_t n) { return 8u + n / 256u; }
	// larger radius first, as an ascending integer: for non-negative floats the order of sqrt(r^2) is the order of the bits of r^2
	RT_HIP_LBVH_FN uint32_t large_key(float r2) { return ~bits_of(r2); }

	RT_HIP_LBVH_FN uint32_t spread3(uint32_t v) // 10 bits, two zeros between neighbours
	{
		v = (v | (v << 16)) & 0x030000FFu;
		v = (v | (v << 8)) & 0x0300F00Fu;
		v = (v | (v << 4)) & 0x030C30C3u;
		v = (v | (v << 2)) & 0x09249249u;
		return v;
	}
	// 10 bits per axis inside the tree spheres' centre bounds; x owns the highest bit of each triple
	RT_HIP_LBVH_FN uint32_t morton30(const float c[3], const float cmin[3], const float cmax[3])
	{
		uint32_t q[3];
		for (int j = 0; j < 3; j++)
		{
			const double width = static_cast<double>(cmax[j]) - static_cast<double>(cmin[j]);
			q[j] = 0u;
			if (width > 0.0)
			{
				const double t = (static_cast<double>(c[j]) - static_cast<double>(cmin[j])) / width * 1024.0;
				q[j] = t >= 1023.0 ? 1023u : (t > 0.0 ? static_cast<uint32_t>(t) : 0u);
			}
		}
		return (spread3(q[0]) << 2) | (spread3(q[1]) << 1) | spread3(q[2]);
	}

	// inner-node levels a subtree of n spheres needs at least (bvh.cpp, levels_needed)
	RT_HIP_LBVH_FN uint32_t levels_needed(uint32_t n)
	{
		const uint32_t leaves = (n + leaf_spheres - 1u) / leaf_spheres;
		uint32_t levels = 0;
		while ((1ull << levels) < leaves)
			levels++;
		return levels;
	}
	RT_HIP_LBVH_FN uint32_t leaf_link(uint32_t first, uint32_t count) { return leaf_bit | ((count - 1u) << 29) | first; }
	RT_HIP_LBVH_FN uint64_t key_at(const uint32_t* morton, const uint32_t* index, uint32_t p) { return (static_cast<uint64_t>(morton[p]) << 32) | index[p]; }

	// Where to cut the sorted range [first, first + count), count > 4, whose node sits at inner level `level` (1 = root): in front
	// of the first key that has the range's highest differing key bit set — if both halves fit the levels left, the rule of
	// bvh.cpp's split — and in the middle otherwise, which always fits.  Returns the left half's size, 1 .. count - 1.
	RT_HIP_LBVH_FN uint32_t choose_cut(const uint32_t* morton, const uint32_t* index, uint32_t first, uint32_t count, uint32_t level)
	{
		const uint64_t differing = key_at(morton, index, first) ^ key_at(morton, index, first + count - 1u); // (keys are unique: not 0)
		const uint64_t bit = 1ull << (63 - __builtin_clzll(differing));
		uint32_t lo = first, hi = first + count - 1u; // the bit is clear at lo and set at hi
		while (hi - lo > 1u)
		{
			const uint32_t mid = lo + (hi - lo) / 2u;
			if (key_at(morton, index, mid) & bit)
				hi = mid;
			else
				lo = mid;
		}
		const uint32_t cut = hi - first, room = max_depth - level;
		if (levels_needed(cut) > room || levels_needed(count - cut) > room)
			return count / 2u;
		return cut;
	}

	// the ball around the tree from its box (bvh.cpp:242-251): the centre rounded to binary32, the radius to its farthest corner rounded up
	RT_HIP_LBVH_FN void ball_of(const float lo[3], const float hi[3], float out[4])
	{
		double r2 = 0.0;
		for (int j = 0; j < 3; j++)
		{
			out[j] = static_cast<float>(0.5 * (static_cast<double>(lo[j]) + hi[j]));
			const double a = static_cast<double>(out[j]) - lo[j], b = static_cast<double>(hi[j]) - out[j];
			const double reach = a > b ? a : b;
			r2 += reach * reach;
		}
		out[3] = up(__builtin_sqrt(r2) * (1.0 + 0x1p-40));
	}
}
}
