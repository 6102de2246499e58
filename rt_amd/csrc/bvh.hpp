// rt_amd/csrc/bvh.hpp — the sphere hierarchy of RT_HIP_FLAG_BVH: its layout (shared with the device traversal, bvh_scan.hpp)
// and the host builder (bvh.cpp, plain C++17: it is built into librt_hip.so and into the test-only librt_hip_kat.so).
//
// A binary tree over the spheres' boxes (centre -/+ sqrt(r^2), rounded outward), built by binned SAH with leaves of at most
// four spheres.  Node k is four float4s, 64 bytes: (box A min, link A), (box A max, link B), (box B min, 0), (box B max, 0);
// a link is a node index, or bvh_leaf_bit | (count - 1) << 29 | first for a leaf of `count` spheres at slots first ..
// first + count - 1 of the leaf-ordered table.  Every inner node has two non-empty children.
// Spheres whose box is large next to the scene (the ground sphere of rt's fields), and spheres that are not finite, stay out of
// the tree: the ALWAYS list, scanned linearly by every query.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

namespace rt_hip
{
	// inner-node levels on any root-to-leaf path, by construction (median splits where SAH would go deeper) = the traversal's
	// stack entries per lane
	constexpr uint32_t bvh_max_depth = 24;
	constexpr uint32_t bvh_leaf_spheres = 4;
	constexpr uint32_t bvh_leaf_bit = 1u << 31;
	constexpr uint32_t bvh_max_tree_spheres = bvh_leaf_spheres << bvh_max_depth; // (2^26; and first < 2^29 in a leaf link)

	struct bvh_host
	{
		std::vector<float> nodes;	   // 16 words per node (links as bits)
		std::vector<float> spheres;	   // 4 per tree sphere in leaf order: bit copies of the (c, r^2) the linear kernels read
		std::vector<uint32_t> order;   // original index of each leaf slot
		std::vector<uint32_t> always;  // original indices of the spheres outside the tree, ascending
		uint32_t root = 0;			   // link of the root: node 0, or one leaf when the tree holds at most four spheres
		uint32_t depth = 0;			   // inner-node levels of the deepest path
		float centre[3] = { 0, 0, 0 }; // ball around every tree sphere: |c - centre| + sqrt(r^2) <= radius (the cull bound's C, R)
		float radius = 0;
	};

	// `geometry` = n float4s (cx, cy, cz, r^2), the primitive table as uploaded.  Deterministic: the same floats give the same
	// bytes.  False (with the reason) only for more than bvh_max_tree_spheres spheres in the tree.
	bool build_bvh(const float* geometry, uint32_t n, bvh_host& out, std::string& why);
}
