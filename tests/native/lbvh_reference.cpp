// tests/native/lbvh_reference.cpp — the device builder of the sphere hierarchy (rt_amd/csrc/bvh_build.hip) restated serially over
// the same per-element header (rt_amd/csrc/bvh_build.hpp), built with g++ alone (tests/test_bvh_lbvh_reference.py): the builder's
// CPU test, and the byte-for-byte target of the GPU test (tests/test_gpu_bvh_device_build.py).
//
//   lbvh_reference IN OUT
//   IN:  uint32 n, then n x 4 float32 (cx, cy, cz, r^2): the sphere rows of the primitive table
//   OUT: uint32 counts[5] = { node slots, tree spheres, always spheres, depth, root link }, then nodes (16 words each), order,
//        spheres (4 floats per leaf slot), always, bound (4 floats) — what rt_hip_kat_bvh_build_device returns
#include "../../rt_amd/csrc/bvh_build.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace rt_hip::lbvh;

namespace
{
	struct tree
	{
		std::vector<uint32_t> nodes, order, always;
		std::vector<float> spheres;
		float bound[4] = { 0, 0, 0, 0 };
		uint32_t root = 0, depth = 0;
	};

	struct range
	{
		uint32_t first, count, parent_word;
	};

	void put(std::vector<uint32_t>& nodes, uint32_t word, float f) { nodes[word] = bits_of(f); }

	tree build(const float* g, uint32_t n)
	{
		tree t;
		// classify: tame spheres and the extent of their centres
		std::vector<char> is_tame(n), out(n, 0);
		float cmin[3] = { 0, 0, 0 }, cmax[3] = { 0, 0, 0 };
		bool any = false;
		for (uint32_t i = 0; i < n; i++)
			if ((is_tame[i] = tame(g + 4 * i)))
			{
				for (int j = 0; j < 3; j++)
				{
					cmin[j] = any ? min_of(cmin[j], g[4 * i + j]) : g[4 * i + j];
					cmax[j] = any ? max_of(cmax[j], g[4 * i + j]) : g[4 * i + j];
				}
				any = true;
			}
		const double extent = any ? extent_of(cmin, cmax) : 0.0;
		// the large spheres: at most the cap leaves the tree, smallest (key, index) first
		std::vector<uint64_t> big;
		for (uint32_t i = 0; i < n; i++)
			if (is_tame[i] && large(g[4 * i + 3], extent))
				big.push_back((static_cast<uint64_t>(large_key(g[4 * i + 3])) << 32) | i);
		std::sort(big.begin(), big.end());
		big.resize(std::min<size_t>(big.size(), large_cap(n)));
		for (const uint64_t k : big)
			out[static_cast<uint32_t>(k)] = 1;
		// the tree's spheres: centre bounds, the box of all their boxes, keys
		float tmin[3] = { 0, 0, 0 }, tmax[3] = { 0, 0, 0 }, blo[3] = { 0, 0, 0 }, bhi[3] = { 0, 0, 0 };
		std::vector<uint32_t> members;
		for (uint32_t i = 0; i < n; i++)
		{
			if (!is_tame[i] || out[i])
			{
				t.always.push_back(i);
				continue;
			}
			float lo[3], hi[3];
			sphere_box(g + 4 * i, lo, hi);
			for (int j = 0; j < 3; j++)
			{
				const bool first = members.empty();
				tmin[j] = first ? g[4 * i + j] : min_of(tmin[j], g[4 * i + j]);
				tmax[j] = first ? g[4 * i + j] : max_of(tmax[j], g[4 * i + j]);
				blo[j] = first ? lo[j] : min_of(blo[j], lo[j]);
				bhi[j] = first ? hi[j] : max_of(bhi[j], hi[j]);
			}
			members.push_back(i);
		}
		const uint32_t n_tree = static_cast<uint32_t>(members.size());
		if (!n_tree)
			return t;
		std::vector<uint64_t> keys;
		for (const uint32_t i : members)
			keys.push_back((static_cast<uint64_t>(morton30(g + 4 * i, tmin, tmax)) << 32) | i);
		std::sort(keys.begin(), keys.end());
		std::vector<uint32_t> morton(n_tree);
		t.order.resize(n_tree);
		for (uint32_t k = 0; k < n_tree; k++)
		{
			morton[k] = static_cast<uint32_t>(keys[k] >> 32);
			t.order[k] = static_cast<uint32_t>(keys[k]);
			t.spheres.insert(t.spheres.end(), g + 4 * t.order[k], g + 4 * t.order[k] + 4);
		}
		ball_of(blo, bhi, t.bound);
		if (n_tree <= leaf_spheres)
		{
			t.root = leaf_link(0, n_tree);
			return t;
		}
		// topology, level by level: node = cut position - 1
		t.nodes.assign(static_cast<size_t>(n_tree - 1) * 16, 0u);
		std::vector<std::vector<uint32_t>> nodes_of_level(max_depth + 2);
		std::vector<range> level = { { 0, n_tree, 0xFFFFFFFFu } }, next;
		for (uint32_t l = 1; !level.empty(); l++)
		{
			t.depth = l;
			next.clear();
			for (const range& r : level)
			{
				const uint32_t cut = choose_cut(morton.data(), t.order.data(), r.first, r.count, l), node = r.first + cut - 1;
				nodes_of_level[l].push_back(node);
				if (r.parent_word == 0xFFFFFFFFu)
					t.root = node;
				else
					t.nodes[r.parent_word] = node;
				const uint32_t first[2] = { r.first, r.first + cut }, count[2] = { cut, r.count - cut };
				for (int c = 0; c < 2; c++)
				{
					const uint32_t word = node * 16 + (c ? 7 : 3);
					if (count[c] <= leaf_spheres)
						t.nodes[word] = leaf_link(first[c], count[c]);
					else
						next.push_back({ first[c], count[c], word });
				}
			}
			level.swap(next);
		}
		// boxes, deepest level first: a child's box is the union of its spheres' boxes
		for (uint32_t l = t.depth; l >= 1; l--)
			for (const uint32_t node : nodes_of_level[l])
				for (int c = 0; c < 2; c++)
				{
					const uint32_t link = t.nodes[node * 16 + (c ? 7 : 3)];
					float lo[3], hi[3];
					if (link & leaf_bit)
					{
						const uint32_t first = link & ((1u << 29) - 1u), count = ((link >> 29) & 3u) + 1u;
						for (uint32_t k = 0; k < count; k++)
						{
							float slo[3], shi[3];
							sphere_box(&t.spheres[4 * (first + k)], slo, shi);
							for (int j = 0; j < 3; j++)
								lo[j] = k ? min_of(lo[j], slo[j]) : slo[j], hi[j] = k ? max_of(hi[j], shi[j]) : shi[j];
						}
					}
					else
						for (int j = 0; j < 3; j++)
						{
							lo[j] = min_of(float_of(t.nodes[link * 16 + j]), float_of(t.nodes[link * 16 + 8 + j]));
							hi[j] = max_of(float_of(t.nodes[link * 16 + 4 + j]), float_of(t.nodes[link * 16 + 12 + j]));
						}
					for (int j = 0; j < 3; j++)
					{
						put(t.nodes, node * 16 + (c ? 8 : 0) + j, lo[j]);
						put(t.nodes, node * 16 + (c ? 12 : 4) + j, hi[j]);
					}
				}
		return t;
	}
}

int main(int argc, char** argv)
{
	if (argc != 3)
		return std::fprintf(stderr, "usage: lbvh_reference IN OUT\n"), 2;
	std::FILE* in = std::fopen(argv[1], "rb");
	uint32_t n = 0;
	if (!in || std::fread(&n, 4, 1, in) != 1)
		return std::fprintf(stderr, "lbvh_reference: cannot read %s\n", argv[1]), 1;
	std::vector<float> g(static_cast<size_t>(n) * 4);
	if (n && std::fread(g.data(), 16, n, in) != n)
		return std::fprintf(stderr, "lbvh_reference: %s is short\n", argv[1]), 1;
	std::fclose(in);
	if (n > max_spheres)
		return std::fprintf(stderr, "lbvh_reference: more than 2^26 spheres\n"), 1;
	const tree t = build(g.data(), n);
	std::FILE* out = std::fopen(argv[2], "wb");
	if (!out)
		return std::fprintf(stderr, "lbvh_reference: cannot write %s\n", argv[2]), 1;
	const uint32_t counts[5] = { static_cast<uint32_t>(t.nodes.size() / 16), static_cast<uint32_t>(t.order.size()), static_cast<uint32_t>(t.always.size()), t.depth, t.root };
	std::fwrite(counts, 4, 5, out);
	std::fwrite(t.nodes.data(), 4, t.nodes.size(), out);
	std::fwrite(t.order.data(), 4, t.order.size(), out);
	std::fwrite(t.spheres.data(), 4, t.spheres.size(), out);
	std::fwrite(t.always.data(), 4, t.always.size(), out);
	std::fwrite(t.bound, 4, 4, out);
	return std::fclose(out) == 0 ? 0 : 1;
}
