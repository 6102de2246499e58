// rt_amd/csrc/passes.hip — a frame in resumable passes behind the drop-in call (rt_hip_render_progressive): every call
// traces the next pass_samples samples of every pixel onto the context's accumulator and delivers the frame as it then stands — the
// one-shot frame at samples_done samples per pixel, bit for bit.  Which samples those are, and whether the accumulation in flight is
// still the caller's frame, is progressive.cpp's business (next_pass, host-only); the launch is render_device's with a pass
// (render.hip); the frame's way to the caller is the carried one (carried_frame, frame_call.hip).
#include "internal.hpp"

#include <algorithm>
#include <cstring>
#include <exception>

using namespace rt_hip;

extern "C" rt_hip_status rt_hip_render_progressive(rt_hip_ctx* ctx,
													   const rt_hip_scene* scene,
													   uint32_t* pixels_rgba8888,
													   uint32_t width,
													   uint32_t height,
													   uint64_t seed,
													   uint32_t flags,
													   uint32_t pass_samples,
													   float* rgb_f32,
													   rt_hip_stats* stats,
													   rt_hip_progress* out_progress)
{
	const auto entered = std::chrono::steady_clock::now();
	if (!ctx || !scene || !pixels_rgba8888)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_render_progressive: NULL argument");
	if (!width || !height)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_render_progressive: empty frame %ux%u", width, height);
	if (const rt_hip_status st = single_context_only("rt_hip_render_progressive", ctx))
		return st;
	if (const char* const refused = refused_pass_flag(flags))
		return fail(RT_HIP_UNSUPPORTED, "rt_hip_render_progressive: %s is not available for passes (0x%x): they take RT_HIP_FLAG_SM_MATERIALS, RT_HIP_FLAG_BVH, RT_HIP_FLAG_BVH_DEVICE_BUILD and RT_HIP_FLAG_STATS", refused, flags);
	if (scene->samples_per_pixel > pass_max_samples_per_pixel)
		return fail(RT_HIP_UNSUPPORTED, "rt_hip_render_progressive: %u samples per pixel: the samples' random windows alias beyond %u", scene->samples_per_pixel, pass_max_samples_per_pixel);
	const size_t pixels = static_cast<size_t>(width) * height;
	const size_t frame_bytes = pixels * sizeof(uint32_t), rgb_bytes = pixels * 3 * sizeof(float);
	const bool keep_stats = stats || (flags & RT_HIP_FLAG_STATS);
	try
	{
		RT_HIP_TRY(hipSetDevice(ctx->device));
		track_frame_buffer(ctx, pixels_rgba8888, frame_bytes, false); // (a page-lock an earlier rt_hip_render took on the caller's buffer is dropped)

		scene_request request;
		if (const rt_hip_status st = resident_scene(ctx, scene, request))
			return st;

		// which samples this call traces: the next of the accumulation in flight, or the first of a new one
		const pass_request wanted = { frame_key_of(request, scene, width, height, seed, flags & pass_frame_flags), pass_samples };
		const pass_step step = next_pass(ctx->progressive, wanted);
		if (step.restart)
		{
			ctx->progressive = pass_state{}; // (nothing in flight until the first pass has succeeded)
			ctx->progressive_passes = 0;
		}
		rt_hip_progress progress{};
		progress.samples_total = scene->samples_per_pixel;
		progress.restarted = step.restart ? 1u : 0u;

		carried_frame frame(ctx, pixels_rgba8888, rgb_f32, pixels);
		if (const rt_hip_status st = frame.open("rt_hip_render_progressive"))
			return st;

		if (!step.n_samples)
		{
			// A finished accumulation: nothing is launched.  The finished frame was kept on the host; its float mean is the accumulator
			// over the sample count — the fold's own division, correctly rounded on either side of the bus.
			if (ctx->progressive_frame.size() != pixels)
				return fail(RT_HIP_RUNTIME_ERROR, "rt_hip_render_progressive: the finished frame was not kept");
			frame.delivery->carrier.copy(pixels_rgba8888, ctx->progressive_frame.data(), frame_bytes);
			if (rgb_f32)
			{
				RT_HIP_TRY(ctx->staging_rgb.reserve(rgb_bytes));
				RT_HIP_TRY(hipMemcpyAsync(ctx->staging_rgb.ptr, ctx->accum.ptr, rgb_bytes, hipMemcpyDeviceToHost, ctx->stream));
				RT_HIP_TRY(hipStreamSynchronize(ctx->stream));
				const float* const sums = ctx->staging_rgb.as<float>();
				const float n = static_cast<float>(scene->samples_per_pixel);
				for (size_t i = 0; i < pixels * 3; i++)
					rgb_f32[i] = sums[i] / n;
			}
			nothing_launched(ctx);
			progress.samples_done = ctx->progressive.samples_done;
			progress.passes = ctx->progressive_passes;
			if (out_progress)
				*out_progress = progress;
			if (stats)
				*stats = ctx->stats;
			return ok();
		}

		RT_HIP_TRY(ctx->accum.reserve(rgb_bytes)); // (grows only where an accumulation starts: the frame's size is part of its key)

		if (const rt_hip_status st = frame.begin())
			return st;
		// a pass that fails leaves the accumulator in an unknown state: nothing is in flight from here until it has succeeded
		const pass_state before = ctx->progressive;
		ctx->progressive = pass_state{};
		const render_pass pass = { step.first_sample, step.n_samples, ctx->accum.as<float>() };
		if (const rt_hip_status st = render_device(ctx, width, height, seed, flags & pass_flag_mask, nullptr, frame.d_frame, frame.d_rgb, ctx->stream, false, keep_stats, true, &pass))
			return st;
		frame.launched();
		if (const rt_hip_status st = frame.deliver(keep_stats ? ctx->render_end : nullptr))
			return st;

		ctx->progressive = before;
		ctx->progressive.started = true;
		ctx->progressive.key = wanted.key;
		ctx->progressive.samples_done = step.first_sample + step.n_samples;
		ctx->progressive_passes++;
		if (step.complete) // later calls deliver this frame again without a launch
			ctx->progressive_frame.assign(pixels_rgba8888, pixels_rgba8888 + pixels);
		progress.samples_done = ctx->progressive.samples_done;
		progress.passes = ctx->progressive_passes;
		if (out_progress)
			*out_progress = progress;

		return frame.account(entered, stats);
	}
	catch (const std::exception& e) // nothing may propagate through the C boundary
	{
		return fail(RT_HIP_RUNTIME_ERROR, "rt_hip_render_progressive: %s", e.what());
	}
}
