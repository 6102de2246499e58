// rt_amd/csrc/box_bvh.cpp — host builder of the box hierarchy (box_bvh.hpp).  Plain C++17, no HIP: librt_hip.so builds a tree on
// the first RT_HIP_FLAG_BOX_BVH frame of a scene, and the test-only library builds the same tree for the CPU suite.
// A sibling of bvh.cpp rather than a sharer of its code: the sphere trees' bytes are pinned (tests/test_bvh_build.py), and what
// differs here — extents taken as they are instead of rounded outward, no ball, eight floats per leaf slot — runs through the
// whole builder.
#include "box_bvh.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace rt_hip
{
	namespace
	{
		struct extent
		{
			float lo[3], hi[3];
			void empty()
			{
				for (int j = 0; j < 3; j++)
					lo[j] = INFINITY, hi[j] = -INFINITY;
			}
			void grow(const extent& b)
			{
				for (int j = 0; j < 3; j++)
					lo[j] = std::min(lo[j], b.lo[j]), hi[j] = std::max(hi[j], b.hi[j]);
			}
			double half_area() const
			{
				const double x = static_cast<double>(hi[0]) - lo[0], y = static_cast<double>(hi[1]) - lo[1], z = static_cast<double>(hi[2]) - lo[2];
				return x * y + y * z + z * x;
			}
		};

		// inner-node levels a subtree of n boxes needs at least (median splits): ceil(log2(ceil(n / 4)))
		uint32_t levels_needed(uint32_t n)
		{
			uint32_t leaves = (n + bvh_leaf_spheres - 1) / bvh_leaf_spheres, levels = 0;
			while ((1ull << levels) < leaves)
				levels++;
			return levels;
		}

		struct builder
		{
			const float* bounds;
			std::vector<extent> extents; // per scene index
			std::vector<float> centroid; // 3 per scene index
			box_bvh_host& out;

			void put_extent(uint32_t node, int which, const extent& b)
			{
				float* const n = &out.nodes[static_cast<size_t>(node) * 16];
				std::memcpy(n + (which == 0 ? 0 : 8), b.lo, sizeof(b.lo));
				std::memcpy(n + (which == 0 ? 4 : 12), b.hi, sizeof(b.hi));
			}
			void put_link(uint32_t node, int which, uint32_t link) { std::memcpy(&out.nodes[static_cast<size_t>(node) * 16 + (which == 0 ? 3 : 7)], &link, 4); }

			extent union_of(const uint32_t* ids, uint32_t n) const
			{
				extent b;
				b.empty();
				for (uint32_t i = 0; i < n; i++)
					b.grow(extents[ids[i]]);
				return b;
			}

			// where to cut ids[0 .. n) into [0, cut) and [cut, n), reordering ids; level = this node's inner level (1 = root)
			uint32_t split(uint32_t* ids, uint32_t n, uint32_t level)
			{
				float cmin[3] = { INFINITY, INFINITY, INFINITY }, cmax[3] = { -INFINITY, -INFINITY, -INFINITY };
				for (uint32_t i = 0; i < n; i++)
					for (int j = 0; j < 3; j++)
						cmin[j] = std::min(cmin[j], centroid[ids[i] * 3 + j]), cmax[j] = std::max(cmax[j], centroid[ids[i] * 3 + j]);
				int axis = 0;
				for (int j = 1; j < 3; j++)
					if (static_cast<double>(cmax[j]) - cmin[j] > static_cast<double>(cmax[axis]) - cmin[axis])
						axis = j;
				const double width = static_cast<double>(cmax[axis]) - cmin[axis];
				const uint32_t room = bvh_max_depth - level; // inner levels left for each child
				if (width > 0.0)
				{
					// binned SAH: 16 bins over the centroids' extent on the widest axis
					constexpr int bins = 16;
					extent bin_extent[bins];
					uint32_t bin_count[bins] = {};
					for (extent& b : bin_extent)
						b.empty();
					const auto bin_of = [&](uint32_t id)
					{
						const int k = static_cast<int>((static_cast<double>(centroid[id * 3 + axis]) - cmin[axis]) * bins / width);
						return std::min(std::max(k, 0), bins - 1);
					};
					for (uint32_t i = 0; i < n; i++)
					{
						const int k = bin_of(ids[i]);
						bin_extent[k].grow(extents[ids[i]]);
						bin_count[k]++;
					}
					double right_area[bins];
					uint32_t right_count[bins];
					extent acc;
					acc.empty();
					uint32_t count = 0;
					for (int k = bins - 1; k >= 1; k--)
					{
						acc.grow(bin_extent[k]);
						count += bin_count[k];
						right_area[k] = count ? acc.half_area() : 0.0;
						right_count[k] = count;
					}
					acc.empty();
					count = 0;
					int best = -1;
					double best_cost = INFINITY;
					for (int k = 0; k < bins - 1; k++) // cut between bin k and bin k + 1
					{
						acc.grow(bin_extent[k]);
						count += bin_count[k];
						const uint32_t right = right_count[k + 1];
						if (!count || !right || levels_needed(count) > room || levels_needed(right) > room)
							continue;
						const double cost = acc.half_area() * count + right_area[k + 1] * right;
						if (cost < best_cost)
							best_cost = cost, best = k;
					}
					if (best >= 0)
					{
						uint32_t* const mid = std::stable_partition(ids, ids + n, [&](uint32_t id) { return bin_of(id) <= best; });
						return static_cast<uint32_t>(mid - ids);
					}
				}
				// median split by (centroid on the axis, index): a total order, so the halves do not depend on the sort
				std::sort(ids, ids + n, [&](uint32_t a, uint32_t b)
						  {
							  const float ka = centroid[a * 3 + axis], kb = centroid[b * 3 + axis];
							  return ka < kb || (ka == kb && a < b);
						  });
				return n / 2;
			}

			uint32_t leaf(const uint32_t* ids, uint32_t n)
			{
				const uint32_t first = static_cast<uint32_t>(out.order.size());
				for (uint32_t i = 0; i < n; i++)
				{
					out.order.push_back(ids[i]);
					out.corners.insert(out.corners.end(), bounds + static_cast<size_t>(ids[i]) * 8, bounds + static_cast<size_t>(ids[i]) * 8 + 8);
				}
				return bvh_leaf_bit | ((n - 1u) << 29) | first;
			}

			// link of the subtree over ids[0 .. n), n >= 1, whose root sits at inner level `level`
			uint32_t build(uint32_t* ids, uint32_t n, uint32_t level)
			{
				if (n <= bvh_leaf_spheres)
					return leaf(ids, n);
				out.depth = std::max(out.depth, level);
				const uint32_t node = static_cast<uint32_t>(out.nodes.size() / 16);
				out.nodes.resize(out.nodes.size() + 16, 0.0f);
				const uint32_t cut = split(ids, n, level);
				put_extent(node, 0, union_of(ids, cut));
				put_extent(node, 1, union_of(ids + cut, n - cut));
				const uint32_t left = build(ids, cut, level + 1);
				put_link(node, 0, left);
				const uint32_t right = build(ids + cut, n - cut, level + 1);
				put_link(node, 1, right);
				return node;
			}
		};
	}

	bool build_box_bvh(const float* bounds, uint32_t n, box_bvh_host& out, std::string& why)
	{
		out = box_bvh_host{};
		builder b{ bounds, std::vector<extent>(n), std::vector<float>(static_cast<size_t>(n) * 3), out };
		std::vector<uint32_t> tree;
		std::vector<double> half(n, 0.0); // a box's largest half width
		std::vector<bool> in_tree(n, false);
		double cmin[3] = { INFINITY, INFINITY, INFINITY }, cmax[3] = { -INFINITY, -INFINITY, -INFINITY };
		for (uint32_t i = 0; i < n; i++)
		{
			const float* const lo = bounds + static_cast<size_t>(i) * 8;
			const float* const hi = lo + 4;
			bool finite = true;
			for (int j = 0; j < 3; j++)
				finite = finite && std::isfinite(lo[j]) && std::isfinite(hi[j]);
			if (!finite) // (the cull's argument needs NaN-free corners; an infinite one would make every node above it infinite)
				continue;
			in_tree[i] = true;
			extent& e = b.extents[i];
			for (int j = 0; j < 3; j++)
			{
				e.lo[j] = std::min(lo[j], hi[j]);
				e.hi[j] = std::max(lo[j], hi[j]);
				const double centre = 0.5 * (static_cast<double>(e.lo[j]) + e.hi[j]); // (binary64: the sum of two finite floats does not overflow)
				b.centroid[static_cast<size_t>(i) * 3 + j] = static_cast<float>(centre);
				half[i] = std::max(half[i], 0.5 * (static_cast<double>(e.hi[j]) - e.lo[j]));
				cmin[j] = std::min(cmin[j], centre);
				cmax[j] = std::max(cmax[j], centre);
			}
		}
		// Large boxes: a half width above a quarter of the centres' widest extent (a ground slab under a field of blocks).  In the tree
		// such a box would cover every node above it.  At most 8 + n / 256 of them, the largest first — which boxes go where changes the
		// speed of a query, never its answer.  Scenes of up to 32 boxes keep every finite box in the tree: a handful of leaves either way.
		double width = 0.0;
		for (int j = 0; j < 3; j++)
			if (cmax[j] > cmin[j])
				width = std::max(width, cmax[j] - cmin[j]);
		std::vector<uint32_t> large;
		for (uint32_t i = 0; i < n; i++)
			if (n > 32u && width > 0.0 && in_tree[i] && half[i] > width / 4.0) // (no extent among the centres — one box, identical boxes —: nothing to be large next to)
				large.push_back(i);
		std::sort(large.begin(), large.end(), [&](uint32_t a, uint32_t c) { return half[a] > half[c] || (half[a] == half[c] && a < c); });
		large.resize(std::min<size_t>(large.size(), 8u + n / 256u));
		for (const uint32_t i : large)
			in_tree[i] = false;
		for (uint32_t i = 0; i < n; i++)
			(in_tree[i] ? tree : out.always).push_back(i);
		if (tree.size() > box_bvh_max_tree_boxes)
		{
			why = "more than 2^26 boxes for the tree";
			return false;
		}
		if (tree.empty())
			return true;
		out.root = b.build(tree.data(), static_cast<uint32_t>(tree.size()), 1);
		return true;
	}
}
