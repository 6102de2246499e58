// rt_amd/csrc/bvh_build_device.hpp — what bvh_build.hip offers scene.hip (ensure_bvh) and the test-only library (kat.hip):
// the device builder of the sphere hierarchy, RT_HIP_FLAG_BVH_DEVICE_BUILD.
#pragma once

#include "kernels.hpp"

#include <algorithm>
#include <stddef.h>

namespace rt_hip
{
	// the build's own state, at the start of its scratch block (float minima / maxima as `ordered` bits, bvh_build.hpp)
	struct bvh_build_header
	{
		uint32_t cmin[3], cmax[3]; // centres of the tame spheres
		uint32_t tmin[3], tmax[3]; // centres of the tree's spheres
		uint32_t blo[3], bhi[3];   // the box of the tree's boxes
		uint32_t n_large, n_tree;
		uint32_t level_first[26], level_count[26]; // the level queues: where level l's ranges start, how many (l = 1 .. 24)
	};

	// offsets into the two blocks a build of n spheres needs, sized for the worst case (the tree's share of the spheres is known on
	// the device only).  The tree's block: the descriptor, n node slots, n leaf-ordered spheres, n scene indices (order, then the
	// always list).  The scratch block: the header, two (key, value) buffers, flags, digit histograms, the level queues.
	struct bvh_build_sizes
	{
		size_t nodes_at, spheres_at, order_at, block_bytes;
		size_t keys_at, values_at, flags_at, histogram_at, queue_at, scratch_bytes;
	};
	bvh_build_sizes bvh_build_sizes_for(uint32_t n);

	// Enqueues the whole build on `stream`: n <= 2^26 rows of `geometry` (device memory) into `block`, whose first bytes become the
	// device_bvh the BVH kernel is handed.  Both blocks are device memory of at least the sizes above.  Reads nothing back and
	// waits for nothing.
	hipError_t build_bvh_device(const float4* geometry, uint32_t n, void* block, void* scratch, hipStream_t stream);
}
