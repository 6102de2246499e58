// rt_amd/csrc/passes.hip — a frame in resumable passes behind the drop-in call (rt_hip_render_progressive): every call
// traces the next pass_samples samples of every pixel onto the context's accumulator and delivers the frame as it then stands — the
// one-shot frame at samples_done samples per pixel, bit for bit.  Which samples those are, and whether the accumulation in flight is
// still the caller's frame, is progressive.cpp's business (next_pass, host-only); the launch is render_device's with a pass
// (render.hip); the frame's way to the caller is rt_hip_render's (the module-owned page-locked frame, frame.hip).
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
	if (ctx->multi || ctx->group || ctx->world != 1u)
		return fail(RT_HIP_UNSUPPORTED, "rt_hip_render_progressive: contexts from rt_hip_create only (not a multi-GPU, rank or frame-group context)");
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

		const auto scene_t0 = std::chrono::steady_clock::now();
		scene_request request;
		if (const rt_hip_status st = open_request(request, scene))
			return st;
		ctx->phases = rt_hip_phases{};
		if (const rt_hip_status st = make_resident(ctx, request))
			return st;
		ctx->stats.upload_ms = static_cast<float>(seconds_since(scene_t0) * 1e3);

		// which samples this call traces: the next of the accumulation in flight, or the first of a new one
		pass_request wanted{};
		wanted.key.scene_fingerprint = request.print;
		wanted.key.samples_per_pixel = scene->samples_per_pixel, wanted.key.max_bounces = scene->max_bounces;
		std::copy(scene->inverse_view_projection, scene->inverse_view_projection + 16, wanted.key.inverse_view_projection);
		wanted.key.width = width, wanted.key.height = height, wanted.key.seed = seed, wanted.key.flags = flags & pass_frame_flags;
		wanted.pass_samples = pass_samples;
		const pass_step step = next_pass(ctx->progressive, wanted);
		if (step.restart)
		{
			ctx->progressive = pass_state{}; // (nothing in flight until the first pass has succeeded)
			ctx->progressive_passes = 0;
		}
		rt_hip_progress progress{};
		progress.samples_total = scene->samples_per_pixel;
		progress.restarted = step.restart ? 1u : 0u;

		frame_delivery* const delivery = delivery_of(ctx);
		if (!delivery)
			return fail(RT_HIP_RUNTIME_ERROR, "rt_hip_render_progressive: out of host memory");

		if (!step.n_samples)
		{
			// A finished accumulation: nothing is launched.  The finished frame was kept on the host; its float mean is the accumulator
			// over the sample count — the fold's own division, correctly rounded on either side of the bus.
			if (ctx->progressive_frame.size() != pixels)
				return fail(RT_HIP_RUNTIME_ERROR, "rt_hip_render_progressive: the finished frame was not kept");
			delivery->carrier.copy(pixels_rgba8888, ctx->progressive_frame.data(), frame_bytes);
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
			ctx->render_recorded = false;
			ctx->stats.kernel_variant = RT_HIP_KERNEL_NONE;
			ctx->stats.primary_samples = ctx->stats.segments = ctx->stats.sphere_tests = ctx->stats.plane_tests = 0;
			ctx->stats.render_ms = ctx->stats.readback_ms = 0.0f;
			progress.samples_done = ctx->progressive.samples_done;
			progress.passes = ctx->progressive_passes;
			if (out_progress)
				*out_progress = progress;
			if (stats)
				*stats = ctx->stats;
			return ok();
		}

		RT_HIP_TRY(ctx->accum.reserve(rgb_bytes)); // (grows only where an accumulation starts: the frame's size is part of its key)

		// the frame's way to the caller, as in rt_hip_render without RT_HIP_FLAG_PERSISTENT_FRAME (render.hip has the why of each step)
		struct abandon_unless_finished
		{
			frame_delivery* delivery;
			~abandon_unless_finished()
			{
				if (delivery)
					delivery->abandon();
			}
		} staged{ nullptr };
		struct drain_before_abandoning // (declared after `staged`: runs first on every early exit)
		{
			hipStream_t stream;
			bool armed;
			~drain_before_abandoning()
			{
				if (armed && hipStreamSynchronize(stream) != hipSuccess)
					(void)hipGetLastError();
			}
		} drain{ ctx->stream, false };
		uint32_t* d_frame = nullptr;
		if (const rt_hip_status st = delivery->begin(pixels_rgba8888, pixels, &d_frame))
			return st;
		staged.delivery = delivery;
		if (rgb_f32)
		{
			RT_HIP_TRY(ctx->frame_rgb.reserve(rgb_bytes));
			RT_HIP_TRY(ctx->staging_rgb.reserve(rgb_bytes));
		}
		// a pass that fails leaves the accumulator in an unknown state: nothing is in flight from here until it has succeeded
		const pass_state before = ctx->progressive;
		ctx->progressive = pass_state{};
		drain.armed = true;
		const render_pass pass = { step.first_sample, step.n_samples, ctx->accum.as<float>() };
		if (const rt_hip_status st = render_device(ctx, width, height, seed, flags & pass_flag_mask, nullptr, d_frame, rgb_f32 ? ctx->frame_rgb.as<float>() : nullptr, ctx->stream, false, keep_stats, true, &pass))
			return st;
		staged.delivery->launched();
		hipError_t e = hipSuccess;
		if (rgb_f32)
			e = hipMemcpyAsync(ctx->staging_rgb.ptr, ctx->frame_rgb.ptr, rgb_bytes, hipMemcpyDeviceToHost, ctx->stream);
		const auto issued = std::chrono::steady_clock::now();
		if (e == hipSuccess && keep_stats)
			e = hipEventSynchronize(ctx->render_end);
		const auto t0 = std::chrono::steady_clock::now();
		const hipError_t drained = hipStreamSynchronize(ctx->stream);
		drain.armed = drained != hipSuccess;
		RT_HIP_TRY(e);
		RT_HIP_TRY(drained);
		staged.delivery->finish();
		ctx->phases.carrier_bands = static_cast<uint32_t>(staged.delivery->carrier.bands());
		ctx->phases.carrier_bands_early = static_cast<uint32_t>(staged.delivery->carrier.early_bands());
		ctx->phases.carrier_helpers = staged.delivery->carrier.helpers();
		staged.delivery = nullptr;
		if (rgb_f32)
			delivery->carrier.copy(rgb_f32, ctx->staging_rgb.ptr, rgb_bytes);

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

		ctx->stats.readback_ms = keep_stats ? static_cast<float>(seconds_since(t0) * 1e3) : 0.0f;
		ctx->phases.host_issue_ms = static_cast<float>(std::chrono::duration<double>(issued - entered).count() * 1e3);
		ctx->phases.host_wait_ms = static_cast<float>(seconds_since(issued) * 1e3);
		if (keep_stats)
			ctx->phases.render_ms = elapsed_or_zero(ctx->render_begin, ctx->render_end);
		if (stats)
			return rt_hip_stats_fetch(ctx, stats);
		return ok();
	}
	catch (const std::exception& e) // nothing may propagate through the C boundary
	{
		return fail(RT_HIP_RUNTIME_ERROR, "rt_hip_render_progressive: %s", e.what());
	}
}
