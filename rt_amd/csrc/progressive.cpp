// rt_amd/csrc/progressive.cpp — the sequencing of a progressive frame's passes (progressive.hpp): host-only, plain C++17.
#include "progressive.hpp"
#include "launch_plan.hpp" // (sample_chunk)

#include <algorithm>
#include <cstring>

namespace rt_hip
{
	bool same_frame(const frame_key& a, const frame_key& b)
	{
		return a.scene_fingerprint == b.scene_fingerprint && a.samples_per_pixel == b.samples_per_pixel && a.max_bounces == b.max_bounces
			   && std::memcmp(a.inverse_view_projection, b.inverse_view_projection, sizeof a.inverse_view_projection) == 0 // (bit patterns: a NaN equals itself, -0 is not 0)
			   && a.width == b.width && a.height == b.height && a.seed == b.seed && a.flags == b.flags;
	}

	const char* refused_pass_flag(uint32_t flags)
	{
		static const struct
		{
			uint32_t bit;
			const char* name;
		} refused[] = { { RT_HIP_FLAG_FAST, "RT_HIP_FLAG_FAST" },
						{ RT_HIP_FLAG_PREVIEW, "RT_HIP_FLAG_PREVIEW" },
						{ RT_HIP_FLAG_FORCE_TILED, "RT_HIP_FLAG_FORCE_TILED" },
						{ RT_HIP_FLAG_FORCE_RESIDENT, "RT_HIP_FLAG_FORCE_RESIDENT" },
						{ RT_HIP_FLAG_FORCE_STREAMED, "RT_HIP_FLAG_FORCE_STREAMED" },
						{ RT_HIP_FLAG_FORCE_HALF_CHUNKS, "RT_HIP_FLAG_FORCE_HALF_CHUNKS" },
						{ RT_HIP_FLAG_FORCE_WHOLE_CHUNKS, "RT_HIP_FLAG_FORCE_WHOLE_CHUNKS" },
						{ RT_HIP_FLAG_PERSISTENT_FRAME, "RT_HIP_FLAG_PERSISTENT_FRAME" },
						{ RT_HIP_FLAG_BOX_BVH, "RT_HIP_FLAG_BOX_BVH" }, // (named first: it modifies the flag below)
						{ RT_HIP_FLAG_TRACE_BOXES, "RT_HIP_FLAG_TRACE_BOXES" }, // (the box builds have no pass build)
						{ RT_HIP_FLAG_EMISSION, "RT_HIP_FLAG_EMISSION" },		  // (nor have the light builds: progressive and adaptive passes)
						{ RT_HIP_FLAG_DIRECT_LIGHT, "RT_HIP_FLAG_DIRECT_LIGHT" }, // (its modifier, DESIGN.md §3.13: by name, not as an unknown bit)
						{ RT_HIP_FLAG_THIN_LENS, "RT_HIP_FLAG_THIN_LENS" } };	  // (nor have the lens builds)
		for (const auto& flag : refused)
			if (flags & flag.bit)
				return flag.name;
		uint32_t known = pass_flag_mask | RT_HIP_FLAG_STATS;
		for (const auto& flag : refused)
			known |= flag.bit;
		return (flags & ~known) ? "unknown flag bits" : nullptr;
	}

	pass_step next_pass(const pass_state& state, const pass_request& request)
	{
		pass_step step{};
		step.restart = !state.started || !same_frame(state.key, request.key);
		const uint32_t total = request.key.samples_per_pixel;
		step.first_sample = step.restart ? 0u : std::min(state.samples_done, total);
		const uint32_t left = total - step.first_sample;
		// whole chunks (a pass continues the chunk-wise fold: it cannot end inside a chunk), in 64 bits: pass_samples may be anything
		const uint64_t rounded = (static_cast<uint64_t>(request.pass_samples) + sample_chunk - 1u) / sample_chunk * sample_chunk;
		step.n_samples = request.pass_samples ? static_cast<uint32_t>(std::min<uint64_t>(rounded, left)) : left;
		step.complete = step.first_sample + step.n_samples == total;
		return step;
	}
}
