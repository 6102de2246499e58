// rt_amd/csrc/pixel_output.hpp — where a finished pixel goes and what is counted on the way: the row arithmetic of a rank's compact
// buffer (global_row, output_row: every render_queue build, and preview_frame), finish_pixel (mean, square root, pack, store: every
// build that finishes pixels — all but the adaptive ones), parked_samples (the half-chunk builds' fold) and add_segments (every build).
#pragma once

#include "contract.hpp"
#include "kernels.hpp"

namespace rt_hip
{
	// image row of row `local_row` of this rank's compact buffer (rt_hip_partition).  All branches are wave-uniform.
	__device__ __forceinline__ uint32_t global_row(uint32_t local_row, const frame_params& p)
	{
		if (p.world == 1u)
			return local_row; // the whole frame: no arithmetic at all
		if (p.stripe_shift != 0xFFFFFFFFu) // stripes of 2^k rows (the default, 8): shifts instead of a division
			return ((((local_row >> p.stripe_shift) * p.world) + p.rank) << p.stripe_shift) | (local_row & ((1u << p.stripe_shift) - 1u));
		return ((local_row / p.stripe_rows) * p.world + p.rank) * p.stripe_rows + (local_row % p.stripe_rows);
	}

	// row of the output buffers that local row `ly` of this rank is written to (wave-uniform branch)
	__device__ __forceinline__ uint32_t output_row(uint32_t ly, const frame_params& p) { return p.frame_rows ? global_row(ly, p) : ly; }

	// :195-200 — mean, sqrt "gamma", pack, store
	__device__ __forceinline__ void finish_pixel(vec3 colour, const frame_params& p, uint32_t lx, uint32_t ly, uint32_t* out_rgba, float* out_rgb)
	{
		const vec3 mean = pixel_mean(colour, static_cast<float>(p.samples_per_pixel));
		const size_t o = static_cast<size_t>(output_row(ly, p)) * p.width + lx;
		if (out_rgb)
		{
			out_rgb[o * 3 + 0] = mean.x;
			out_rgb[o * 3 + 1] = mean.y;
			out_rgb[o * 3 + 2] = mean.z;
		}
		// A system-scope store: written through to memory at once.  When the frame is the caller's page-locked back buffer
		// (rt_hip_render) the pixels then cross PCIe while the rest of the frame is still being traced; an ordinary store
		// would sit in L2 until the end-of-kernel write-back and put the whole 8 MB transfer behind the kernel
		// (measured: + 0.10-0.14 ms per frame, profiles/r02/frame_store_ab.txt).  For a frame in HBM it costs nothing.
		__hip_atomic_store(&out_rgba[o], pack_mean(mean), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
	}

	// half-chunks: how many samples of chunk `chunk` lie in its second half (indices chunk * 16 + 8 ..)
	__device__ __forceinline__ uint32_t parked_samples(uint32_t samples_per_pixel, uint32_t chunk)
	{
		const uint32_t first = chunk * sample_chunk + sample_chunk / 2u;
		return samples_per_pixel > first ? min(samples_per_pixel - first, sample_chunk / 2u) : 0u;
	}

	// `segments` = the wave's count (wave-uniform: kept in a scalar register, one popcount of the tracing lanes per trip)
	__device__ __forceinline__ void add_segments(device_counters* counters, unsigned long long segments)
	{
		if ((threadIdx.x & 63u) == 0 && segments)
			atomicAdd(&counters->segments[(blockIdx.x + blockIdx.y * 7u + (threadIdx.x >> 6)) % device_counters::segment_counters], segments);
	}
}
