// tests/native/box_bvh_sanitize.cpp — `make sanitize-box-bvh`: the box hierarchy's host builder (rt_amd/csrc/box_bvh.cpp) behind a main() of
// its own, compiled with it under AddressSanitizer and UndefinedBehaviorSanitizer and run at once.  CPU only; nothing here is loaded
// into python.  The inputs are those of tests/test_box_bvh_build.py — 0, 1, 4, 5, 257 and 5 000 boxes, 64 identical boxes, the chain
// that reaches depth 24, boxes with lo > hi, boxes with NaN and infinite corners, a large slab — and every tree is checked the way the
// test checks it: every box once, leaf slots bit copies, child boxes the exact unions of what lies below them, depth within the
// stack, two builds the same bytes.
#include "../../rt_amd/csrc/box_bvh.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace rt_hip;

namespace
{
	int failures = 0;
#define EXPECT(cond, ...)                                                                                                              \
	do                                                                                                                                 \
	{                                                                                                                                  \
		if (!(cond))                                                                                                                   \
		{                                                                                                                              \
			std::printf("FAILED %s: ", name);                                                                                          \
			std::printf(__VA_ARGS__);                                                                                                  \
			std::printf("\n");                                                                                                         \
			failures++;                                                                                                                \
		}                                                                                                                              \
	}                                                                                                                                  \
	while (false)

	struct span
	{
		float lo[3], hi[3];
		uint32_t depth;
	};

	uint32_t random_state = 12345u;
	float uniform(float lo, float hi)
	{
		random_state = random_state * 1664525u + 1013904223u;
		return lo + (hi - lo) * static_cast<float>(random_state >> 8) * (1.0f / 16777216.0f);
	}

	// (centre, extents, material) rows -> the pairs as the upload derives them
	std::vector<float> pairs_of(const std::vector<float>& rows)
	{
		const size_t n = rows.size() / 7;
		std::vector<float> bounds(n * 8, 0.0f);
		for (size_t i = 0; i < n; i++)
		{
			for (int j = 0; j < 3; j++)
			{
				bounds[i * 8 + j] = rows[i * 7 + j] - rows[i * 7 + 3 + j];
				bounds[i * 8 + 4 + j] = rows[i * 7 + j] + rows[i * 7 + 3 + j];
			}
			const uint32_t material = static_cast<uint32_t>(rows[i * 7 + 6]);
			std::memcpy(&bounds[i * 8 + 3], &material, 4);
		}
		return bounds;
	}

	span walk(const char* name, const box_bvh_host& t, const std::vector<float>& bounds, uint32_t link, std::vector<uint32_t>& seen)
	{
		span s{ { INFINITY, INFINITY, INFINITY }, { -INFINITY, -INFINITY, -INFINITY }, 0 };
		if (link & bvh_leaf_bit)
		{
			const uint32_t first = link & ((1u << 29) - 1u), count = ((link >> 29) & 3u) + 1u;
			EXPECT(first + count <= t.order.size(), "a leaf past the table: %u + %u", first, count);
			for (uint32_t k = first; k < first + count && k < t.order.size(); k++)
			{
				seen[k]++;
				const float* const b = &bounds[static_cast<size_t>(t.order[k]) * 8];
				for (int j = 0; j < 3; j++)
					s.lo[j] = std::min(s.lo[j], std::min(b[j], b[4 + j])), s.hi[j] = std::max(s.hi[j], std::max(b[j], b[4 + j]));
			}
			return s;
		}
		EXPECT(static_cast<size_t>(link) * 16 < t.nodes.size(), "a link past the nodes: %u", link);
		if (static_cast<size_t>(link) * 16 >= t.nodes.size())
			return s;
		const float* const node = &t.nodes[static_cast<size_t>(link) * 16];
		uint32_t links[2];
		std::memcpy(&links[0], node + 3, 4);
		std::memcpy(&links[1], node + 7, 4);
		for (int which = 0; which < 2; which++)
		{
			const span child = walk(name, t, bounds, links[which], seen);
			EXPECT(std::memcmp(node + which * 8, child.lo, 12) == 0 && std::memcmp(node + which * 8 + 4, child.hi, 12) == 0, "node %u child %d is not the exact union of what lies below it", link, which);
			for (int j = 0; j < 3; j++)
				s.lo[j] = std::min(s.lo[j], child.lo[j]), s.hi[j] = std::max(s.hi[j], child.hi[j]);
			s.depth = std::max(s.depth, child.depth + 1u);
		}
		return s;
	}

	box_bvh_host check(const char* name, const std::vector<float>& rows, int want_depth = -1)
	{
		const std::vector<float> bounds = pairs_of(rows);
		const uint32_t n = static_cast<uint32_t>(bounds.size() / 8);
		box_bvh_host t, again;
		std::string why;
		EXPECT(build_box_bvh(bounds.data(), n, t, why), "refused: %s", why.c_str());
		EXPECT(build_box_bvh(bounds.data(), n, again, why), "refused the second time: %s", why.c_str());
		EXPECT(t.nodes.size() == again.nodes.size() && (t.nodes.empty() || std::memcmp(t.nodes.data(), again.nodes.data(), t.nodes.size() * 4) == 0), "two builds differ in their nodes");
		EXPECT(t.corners.size() == again.corners.size() && (t.corners.empty() || std::memcmp(t.corners.data(), again.corners.data(), t.corners.size() * 4) == 0), "two builds differ in their leaf table");
		EXPECT(t.order == again.order && t.always == again.always && t.root == again.root && t.depth == again.depth, "two builds differ");
		std::vector<uint32_t> times(n, 0);
		for (const uint32_t i : t.order)
			if (i < n)
				times[i]++;
		for (const uint32_t i : t.always)
			if (i < n)
				times[i]++;
		EXPECT(t.order.size() + t.always.size() == n && std::all_of(times.begin(), times.end(), [](uint32_t c) { return c == 1u; }), "not every box exactly once");
		EXPECT(std::is_sorted(t.always.begin(), t.always.end()), "the always list is not ascending");
		EXPECT(t.corners.size() == t.order.size() * 8, "the leaf table's size");
		for (size_t k = 0; k < t.order.size() && t.corners.size() == t.order.size() * 8; k++)
		{
			EXPECT(std::memcmp(&t.corners[k * 8], &bounds[static_cast<size_t>(t.order[k]) * 8], 32) == 0, "leaf slot %zu is no bit copy", k);
			for (int j = 0; j < 8; j++)
				if (j != 3 && j != 7)
					EXPECT(std::isfinite(t.corners[k * 8 + j]), "a non-finite corner in the tree (slot %zu)", k);
		}
		EXPECT(t.depth <= bvh_max_depth, "depth %u", t.depth);
		if (!t.order.empty())
		{
			std::vector<uint32_t> seen(t.order.size(), 0);
			const span root = walk(name, t, bounds, t.root, seen);
			EXPECT(root.depth == t.depth, "depth %u reported, %u walked", t.depth, root.depth);
			EXPECT(std::all_of(seen.begin(), seen.end(), [](uint32_t c) { return c == 1u; }), "a leaf slot in no leaf, or in two");
		}
		else
			EXPECT(t.nodes.empty(), "nodes without a tree");
		if (want_depth >= 0)
			EXPECT(static_cast<int>(t.depth) == want_depth, "depth %u, expected %d", t.depth, want_depth);
		std::printf("%-28s %6u boxes: %6zu nodes, %6zu in the tree, %3zu always, depth %2u\n", name, n, t.nodes.size() / 16, t.order.size(), t.always.size(), t.depth);
		return t;
	}

	std::vector<float> field(uint32_t count)
	{
		std::vector<float> rows;
		for (uint32_t i = 0; i < count; i++)
		{
			for (int j = 0; j < 3; j++)
				rows.push_back(uniform(-6.0f, 6.0f));
			for (int j = 0; j < 3; j++)
				rows.push_back(uniform(0.001f, 0.4f));
			rows.push_back(static_cast<float>(i % 4u));
		}
		return rows;
	}
}

int main()
{
	for (const uint32_t count : { 0u, 1u, 4u, 5u, 257u, 5000u })
	{
		char name[32];
		std::snprintf(name, sizeof(name), "field of %u", count);
		const box_bvh_host t = check(name, field(count), count <= 4u ? 0 : (count == 5u ? 1 : -1));
		if (count == 1u || count == 4u)
			EXPECT((t.root & bvh_leaf_bit) && t.nodes.empty(), "the root is no leaf");
	}
	{
		std::vector<float> rows;
		for (int i = 0; i < 64; i++)
			rows.insert(rows.end(), { 1.0f, 2.0f, 3.0f, 0.5f, 0.25f, 0.125f, static_cast<float>(i % 4) });
		check("64 identical boxes", rows, 4);
	}
	for (int axis = 0; axis < 3; axis++)
		for (const float sign : { 1.0f, -1.0f })
		{
			std::vector<float> rows(37 * 9 * 7, 0.0f);
			for (int i = 0; i < 37; i++)
				for (int j = 0; j < 9; j++)
				{
					float* const row = &rows[static_cast<size_t>(i * 9 + j) * 7];
					row[axis] = static_cast<float>(sign * std::pow(16.0, -i) * (1.0 + 0.01 * j));
					row[3] = row[4] = row[5] = static_cast<float>(0.001 * std::pow(16.0, -i));
				}
			char name[32];
			std::snprintf(name, sizeof(name), "chain, axis %d, sign %+.0f", axis, sign);
			check(name, rows, static_cast<int>(bvh_max_depth));
		}
	{
		std::vector<float> rows = field(40);
		for (size_t i = 0; i < 40; i += 3)
			rows[i * 7 + 3] = -rows[i * 7 + 3];
		for (size_t i = 1; i < 40; i += 4)
			rows[i * 7 + 4] = -rows[i * 7 + 4], rows[i * 7 + 5] = -rows[i * 7 + 5];
		const char* const name = "lo above hi";
		const box_bvh_host t = check(name, rows);
		EXPECT(t.always.empty(), "a finite box outside the tree");
	}
	{
		std::vector<float> rows = field(30);
		rows[4 * 7 + 0] = NAN;
		rows[9 * 7 + 4] = INFINITY;
		rows[15 * 7 + 2] = -INFINITY;
		rows[21 * 7 + 5] = NAN;
		rows[22 * 7 + 0] = 3e38f, rows[22 * 7 + 3] = 3e38f; // finite columns, an infinite corner
		const char* const name = "NaN and infinite corners";
		const box_bvh_host t = check(name, rows);
		for (const uint32_t i : { 4u, 9u, 15u, 21u, 22u })
			EXPECT(std::binary_search(t.always.begin(), t.always.end(), i), "box %u is not in the always list", i);
	}
	{
		std::vector<float> rows = { 0.0f, -0.5f, 0.0f, 100.0f, 0.5f, 100.0f, 0.0f };
		const std::vector<float> more = field(300);
		rows.insert(rows.end(), more.begin(), more.end());
		const char* const name = "a slab under a field";
		const box_bvh_host t = check(name, rows);
		EXPECT(std::binary_search(t.always.begin(), t.always.end(), 0u), "the slab is in the tree");
	}
	if (failures)
	{
		std::printf("%d checks FAILED\n", failures);
		return 1;
	}
	std::printf("box_bvh_sanitize: all checks passed\n");
	return 0;
}
