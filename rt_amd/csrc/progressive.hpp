// rt_amd/csrc/progressive.hpp — the sequencing of a progressive frame's passes (rt_hip_render_progressive): which samples the
// next call traces, and whether the accumulation in flight is still the caller's frame or has to start again.  Host-only
// integer policy: plain C++17, no HIP header, built with the host compiler into librt_hip.so and, on the CPU, into
// tests/native/pass_plan_dump (tests/test_pass_plan.py pins every rule).
//
// Why passes are exact: a pixel's value is the fold, in chunk order, of sums of sample_chunk consecutive
// samples, and a sample's random window does not depend on the sample count.  A frame that has folded chunks 0 .. c-1 is the
// one-shot frame of the same scene at 16 c samples per pixel, bit for bit — so a pass is any run of whole chunks.
#pragma once

#include <stdint.h>
#include "../../include/rt_hip.h" // (the render flags)

namespace rt_hip
{
	// Passes exist for the parity contract's tile-per-wave kernels: these flags a pass's launch takes — both entry points
	// accept RT_HIP_FLAG_STATS besides, which asks for timing and is no business of the launch — and every other one is refused by name.
	constexpr uint32_t pass_flag_mask = RT_HIP_FLAG_SM_MATERIALS | RT_HIP_FLAG_BVH | RT_HIP_FLAG_BVH_DEVICE_BUILD;
	// of those, the ones that change the frame (frame_key::flags): the hierarchy's frames are the linear scan's, bit for bit
	constexpr uint32_t pass_frame_flags = RT_HIP_FLAG_SM_MATERIALS;
	// the name of a flag in `flags` that a pass does not take ("unknown flag bits" for a bit without a name); NULL: all accepted
	const char* refused_pass_flag(uint32_t flags);
	// windows of the random streams alias beyond this many samples per pixel: no progressive frame goes further
	constexpr uint32_t pass_max_samples_per_pixel = 1u << 20;

	// everything the pixels of a frame depend on: two calls with equal keys continue one accumulation
	struct frame_key
	{
		uint64_t scene_fingerprint; // of the caller's columns (rt_hip_scene_check)
		uint32_t samples_per_pixel, max_bounces;
		float inverse_view_projection[16]; // compared as bit patterns
		uint32_t width, height;
		uint64_t seed;
		uint32_t flags; // the flags that change the frame (pass_frame_flags): how a bit-identical frame is traced is not one's business
	};
	bool same_frame(const frame_key& a, const frame_key& b);

	// the accumulation in flight: what it was started with, and how far it has come
	struct pass_state
	{
		bool started = false; // false: nothing in flight (a new context, or a pass that failed)
		frame_key key{};
		uint32_t samples_done = 0; // a multiple of sample_chunk, or samples_per_pixel
	};

	struct pass_request
	{
		frame_key key;
		uint32_t pass_samples; // rounded up to whole chunks; 0 = all that is left
	};

	struct pass_step
	{
		bool restart;		   // the key differs from the state's (or nothing was in flight): the accumulation starts again at sample 0
		uint32_t first_sample; // the pass traces samples [first_sample, first_sample + n_samples)
		uint32_t n_samples;	   // 0: the accumulation was finished already, nothing is launched
		bool complete;		   // first_sample + n_samples == samples_per_pixel: the frame after this step is the one-shot frame
	};
	pass_step next_pass(const pass_state& state, const pass_request& request);
}
