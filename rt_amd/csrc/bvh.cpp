// rt_amd/csrc/bvh.cpp — host builder of the sphere hierarchy (bvh.hpp).  Plain C++17, no HIP: librt_hip.so builds a tree on
// the first RT_HIP_FLAG_BVH frame of a scene, and the test-only library builds the same tree for the CPU suite.
#include "bvh.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace rt_hip
{
	namespace
	{
		struct box
		{
			float lo[3], hi[3];
			void empty()
			{
				for (int j = 0; j < 3; j++)
					lo[j] = INFINITY, hi[j] = -INFINITY;
			}
			void grow(const box& b)
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

		// binary32 at or below / at or above a binary64 value
		float down(double v)
		{
			float f = static_cast<float>(v);
			if (static_cast<double>(f) > v)
				f = std::nextafter(f, -INFINITY);
			return f;
		}
		float up(double v)
		{
			float f = static_cast<float>(v);
			if (static_cast<double>(f) < v)
				f = std::nextafter(f, INFINITY);
			return f;
		}

		// inner-node levels a subtree of n spheres needs at least (median splits): ceil(log2(ceil(n / 4)))
		uint32_t levels_needed(uint32_t n)
		{
			uint32_t leaves = (n + bvh_leaf_spheres - 1) / bvh_leaf_spheres, levels = 0;
			while ((1ull << levels) < leaves)
				levels++;
			return levels;
		}

		struct builder
		{
			const float* geometry;
			std::vector<box> boxes;		 // per original index
			std::vector<float> centroid; // 3 per original index
			bvh_host& out;

			void put_box(uint32_t node, int which, const box& b)
			{
				float* const n = &out.nodes[static_cast<size_t>(node) * 16];
				float* const lo = n + (which == 0 ? 0 : 8);
				float* const hi = n + (which == 0 ? 4 : 12);
				std::memcpy(lo, b.lo, sizeof(b.lo));
				std::memcpy(hi, b.hi, sizeof(b.hi));
			}
			void put_link(uint32_t node, int which, uint32_t link) { std::memcpy(&out.nodes[static_cast<size_t>(node) * 16 + (which == 0 ? 3 : 7)], &link, 4); }

			box bounds(const uint32_t* ids, uint32_t n) const
			{
				box b;
				b.empty();
				for (uint32_t i = 0; i < n; i++)
					b.grow(boxes[ids[i]]);
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
				const double extent = static_cast<double>(cmax[axis]) - cmin[axis];
				const uint32_t room = bvh_max_depth - level; // inner levels left for each child
				if (extent > 0.0)
				{
					// binned SAH: 16 bins over the centroids' extent on the widest axis
					constexpr int bins = 16;
					box bin_box[bins];
					uint32_t bin_count[bins] = {};
					for (box& b : bin_box)
						b.empty();
					const auto bin_of = [&](uint32_t id)
					{
						const int k = static_cast<int>((static_cast<double>(centroid[id * 3 + axis]) - cmin[axis]) * bins / extent);
						return std::min(std::max(k, 0), bins - 1);
					};
					for (uint32_t i = 0; i < n; i++)
					{
						const int k = bin_of(ids[i]);
						bin_box[k].grow(boxes[ids[i]]);
						bin_count[k]++;
					}
					double right_area[bins];
					uint32_t right_count[bins];
					box acc;
					acc.empty();
					uint32_t count = 0;
					for (int k = bins - 1; k >= 1; k--)
					{
						acc.grow(bin_box[k]);
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
						acc.grow(bin_box[k]);
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
					out.spheres.insert(out.spheres.end(), geometry + static_cast<size_t>(ids[i]) * 4, geometry + static_cast<size_t>(ids[i]) * 4 + 4);
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
				put_box(node, 0, bounds(ids, cut));
				put_box(node, 1, bounds(ids + cut, n - cut));
				const uint32_t left = build(ids, cut, level + 1);
				put_link(node, 0, left);
				const uint32_t right = build(ids + cut, n - cut, level + 1);
				put_link(node, 1, right);
				return node;
			}
		};
	}

	bool build_bvh(const float* geometry, uint32_t n, bvh_host& out, std::string& why)
	{
		out = bvh_host{};
		builder b{ geometry, std::vector<box>(n), std::vector<float>(static_cast<size_t>(n) * 3), out };
		std::vector<uint32_t> tree;
		std::vector<double> half(n, 0.0);
		// which spheres the tree can take: finite, and small enough that no product of the probe overflows
		double cmin[3] = { INFINITY, INFINITY, INFINITY }, cmax[3] = { -INFINITY, -INFINITY, -INFINITY };
		std::vector<bool> in_tree(n, false);
		for (uint32_t i = 0; i < n; i++)
		{
			const float* const g = geometry + static_cast<size_t>(i) * 4;
			bool tame = g[3] >= 0.0f && g[3] <= 0x1p80f;
			for (int j = 0; j < 3; j++)
				tame = tame && std::fabs(g[j]) <= 0x1p40f; // (a NaN fails)
			if (!tame)
				continue;
			in_tree[i] = true;
			half[i] = std::sqrt(static_cast<double>(g[3])); // the radius the probe's arithmetic is about: sqrt of the float r^2
			box& bx = b.boxes[i];
			for (int j = 0; j < 3; j++)
			{
				bx.lo[j] = down(static_cast<double>(g[j]) - half[i]);
				bx.hi[j] = up(static_cast<double>(g[j]) + half[i]);
				b.centroid[static_cast<size_t>(i) * 3 + j] = g[j];
				cmin[j] = std::min(cmin[j], static_cast<double>(g[j]));
				cmax[j] = std::max(cmax[j], static_cast<double>(g[j]));
			}
		}
		// Large spheres: a radius above a quarter of the centres' widest extent.  In the tree such a sphere would cover every node
		// and widen the cull margin of every query (the margin grows with the tree's bounding ball).  At most 8 + n / 256 of them,
		// the largest first — which spheres go where changes the speed of a query, never its answer.
		double extent = 0.0;
		for (int j = 0; j < 3; j++)
			if (cmax[j] > cmin[j])
				extent = std::max(extent, cmax[j] - cmin[j]);
		std::vector<uint32_t> large;
		for (uint32_t i = 0; i < n; i++)
			if (in_tree[i] && half[i] > extent / 4.0)
				large.push_back(i);
		std::sort(large.begin(), large.end(), [&](uint32_t a, uint32_t c) { return half[a] > half[c] || (half[a] == half[c] && a < c); });
		large.resize(std::min<size_t>(large.size(), 8u + n / 256u));
		for (const uint32_t i : large)
			in_tree[i] = false;
		for (uint32_t i = 0; i < n; i++)
			(in_tree[i] ? tree : out.always).push_back(i);
		if (tree.size() > bvh_max_tree_spheres)
		{
			why = "more than 2^26 spheres for the tree";
			return false;
		}
		if (tree.empty())
			return true;
		// the ball: the tree's box, its centre rounded to binary32, the radius to that centre's farthest corner rounded up
		box all = b.bounds(tree.data(), static_cast<uint32_t>(tree.size()));
		double r2 = 0.0;
		for (int j = 0; j < 3; j++)
		{
			out.centre[j] = static_cast<float>(0.5 * (static_cast<double>(all.lo[j]) + all.hi[j]));
			const double reach = std::max(static_cast<double>(out.centre[j]) - all.lo[j], static_cast<double>(all.hi[j]) - out.centre[j]);
			r2 += reach * reach;
		}
		out.radius = up(std::sqrt(r2) * (1.0 + 0x1p-40));
		out.root = b.build(tree.data(), static_cast<uint32_t>(tree.size()), 1);
		return true;
	}
}
