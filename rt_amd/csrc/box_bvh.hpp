// rt_amd/csrc/box_bvh.hpp — the box hierarchy of RT_HIP_FLAG_BOX_BVH: its layout (shared with the device traversal,
// box_bvh_scan.hpp) and the host builder (box_bvh.cpp, plain C++17: built into librt_hip.so and into the test-only librt_hip_kat.so).
//
// The node layout, the leaf links, bvh_max_depth and the leaf size are the sphere hierarchy's (bvh.hpp): a binary tree built by
// binned SAH with leaves of at most four boxes; node k is four float4s, 64 bytes: (box A min, link A), (box A max, link B),
// (box B min, 0), (box B max, 0); a link is a node index, or bvh_leaf_bit | (count - 1) << 29 | first for a leaf of `count` boxes at
// slots first .. first + count - 1 of the leaf-ordered table.  Every inner node has two non-empty children.
//
// A box's EXTENT is the per-axis min and max of its two corners as uploaded (device_scene::box_bounds): a negative extent gives
// lo > hi there, and hits_box treats that box like the swapped one.  A node's box is the exact union of the extents below it — min and
// max of floats do not round, so nothing is rounded outward, and the traversal's cull needs no padding (box_bvh_scan.hpp).
// Boxes with a non-finite corner, and boxes that are large next to the scene (a ground slab), stay out of the tree: the ALWAYS list,
// scanned linearly by every query.
#pragma once

#include "bvh.hpp"

namespace rt_hip
{
	constexpr uint32_t box_bvh_max_tree_boxes = bvh_max_tree_spheres; // (2^26: leaves of four at the bottom of bvh_max_depth levels; first < 2^29 in a leaf link)

	struct box_bvh_host
	{
		std::vector<float> nodes;	  // 16 words per node (links as bits)
		std::vector<float> corners;	  // 8 per tree box in leaf order: bit copies of its two float4s of box_bounds (the material bits travel with them)
		std::vector<uint32_t> order;  // scene index of each leaf slot
		std::vector<uint32_t> always; // scene indices of the boxes outside the tree, ascending
		uint32_t root = 0;			  // link of the root: node 0, or one leaf when the tree holds at most four boxes
		uint32_t depth = 0;			  // inner-node levels of the deepest path
	};

	// `bounds` = n pairs of float4s, (min corner, material bits) and (max corner, 0), exactly as uploaded.  Deterministic: the same
	// floats give the same bytes.  False (with the reason) only for more than box_bvh_max_tree_boxes boxes in the tree.
	bool build_box_bvh(const float* bounds, uint32_t n, box_bvh_host& out, std::string& why);
}
