// rt_amd/csrc/frame_call.hip — the host-side steps the single-context drop-in calls share: rt_hip_render's single-GPU
// branch, rt_hip_render_progressive, rt_hip_render_adaptive, rt_hip_render_temporal, rt_hip_render_upscaled and
// rt_hip_denoise_progressive.  What a call refuses a context or a set of buffers for, its scene prologue and frame key, and the two ways
// a finished frame reaches the caller's plain memory: carried (carried_frame) and staged (staged_results).  internal.hpp says what each
// step is; the order of the HIP calls in here is the calls' contract.
#include "internal.hpp"

#include <algorithm>

namespace rt_hip
{
rt_hip_status single_context_only(const char* who, const rt_hip_ctx* ctx)
{
	if (ctx->multi || ctx->group || ctx->world != 1u)
		return fail(RT_HIP_UNSUPPORTED, "%s: contexts from rt_hip_create only (not a multi-GPU, rank or frame-group context)", who);
	return ok();
}

rt_hip_status resident_scene(rt_hip_ctx* ctx, const rt_hip_scene* scene, scene_request& request)
{
	const auto scene_t0 = std::chrono::steady_clock::now();
	if (const rt_hip_status st = open_request(request, scene))
		return st;
	ctx->phases = rt_hip_phases{};
	if (const rt_hip_status st = make_resident(ctx, request))
		return st;
	ctx->stats.upload_ms = static_cast<float>(seconds_since(scene_t0) * 1e3);
	return ok();
}

frame_key frame_key_of(const scene_request& request, const rt_hip_scene* scene, uint32_t width, uint32_t height, uint64_t seed, uint32_t flags)
{
	frame_key key{};
	key.scene_fingerprint = request.print;
	key.samples_per_pixel = scene->samples_per_pixel, key.max_bounces = scene->max_bounces;
	std::copy(scene->inverse_view_projection, scene->inverse_view_projection + 16, key.inverse_view_projection);
	key.width = width, key.height = height, key.seed = seed, key.flags = flags;
	return key;
}

rt_hip_status guide_boxes(const char* who, const rt_hip_ctx* ctx, uint32_t flags, bool* trace_boxes)
{
	*trace_boxes = (flags & RT_HIP_FLAG_TRACE_BOXES) && ctx->scene.n_boxes;
	if (*trace_boxes && ctx->scene.n_boxes > box_max_count)
		return fail(RT_HIP_UNSUPPORTED, "%s: RT_HIP_FLAG_TRACE_BOXES traces at most %u boxes, the scene has %u", who, box_max_count, ctx->scene.n_boxes);
	return ok();
}

void nothing_launched(rt_hip_ctx* ctx)
{
	ctx->render_recorded = false;
	ctx->stats.kernel_variant = RT_HIP_KERNEL_NONE;
	ctx->stats.primary_samples = ctx->stats.segments = ctx->stats.sphere_tests = ctx->stats.plane_tests = 0;
	ctx->stats.render_ms = ctx->stats.readback_ms = 0.0f;
}

rt_hip_status refuse_overlaps(const char* who, std::initializer_list<named_buffer> outputs, std::initializer_list<named_buffer> inputs, const char* why, const char* among_outputs)
{
	for (const named_buffer& out : outputs)
		for (const named_buffer& in : inputs)
			if (out.ptr && in.ptr && buffers_overlap(out.ptr, out.bytes, in.ptr, in.bytes))
				return fail(RT_HIP_INVALID_ARGUMENT, "%s: %s overlaps %s (%s)", who, out.name, in.name, why);
	for (const named_buffer* a = outputs.begin(); a != outputs.end(); a++)
		for (const named_buffer* b = a + 1; b != outputs.end(); b++)
			if (a->ptr && b->ptr && buffers_overlap(a->ptr, a->bytes, b->ptr, b->bytes))
				return among_outputs ? fail(RT_HIP_INVALID_ARGUMENT, "%s: %s", who, among_outputs) : fail(RT_HIP_INVALID_ARGUMENT, "%s: %s overlaps %s", who, a->name, b->name);
	return ok();
}

rt_hip_status carried_frame::open(const char* who)
{
	delivery = delivery_of(ctx);
	if (!delivery)
		return fail(RT_HIP_RUNTIME_ERROR, "%s: out of host memory", who);
	return ok();
}

rt_hip_status carried_frame::begin(uint32_t* direct)
{
	d_frame = direct;
	if (!d_frame)
	{
		if (const rt_hip_status st = delivery->begin(pixels_rgba8888, pixels, &d_frame))
			return st;
		scope.carried = delivery;
	}
	if (rgb_f32)
	{
		const size_t rgb_bytes = pixels * 3 * sizeof(float);
		RT_HIP_TRY(ctx->frame_rgb.reserve(rgb_bytes));
		RT_HIP_TRY(ctx->staging_rgb.reserve(rgb_bytes));
		d_rgb = ctx->frame_rgb.as<float>();
	}
	scope.armed = true; // from here on the device may be storing into host memory: no return before the stream has drained
	return ok();
}

rt_hip_status carried_frame::deliver(hipEvent_t end_event, hipError_t e)
{
	const size_t rgb_bytes = pixels * 3 * sizeof(float);
	end = end_event;
	if (e == hipSuccess && rgb_f32) // the float mean lands in the module's own page-locked buffer and is copied on from there
		e = hipMemcpyAsync(ctx->staging_rgb.ptr, ctx->frame_rgb.ptr, rgb_bytes, hipMemcpyDeviceToHost, ctx->stream);
	issued = std::chrono::steady_clock::now();
	if (e == hipSuccess && end)
		e = hipEventSynchronize(end);
	waited_from = std::chrono::steady_clock::now();
	const hipError_t drained = scope.drain();
	RT_HIP_TRY(e);
	RT_HIP_TRY(drained);
	if (scope.carried)
	{
		scope.carried->finish(); // the last tiles' pixels; returns with the whole frame in the caller's buffer
		ctx->phases.carrier_bands = static_cast<uint32_t>(delivery->carrier.bands());
		ctx->phases.carrier_bands_early = static_cast<uint32_t>(delivery->carrier.early_bands());
		ctx->phases.carrier_helpers = delivery->carrier.helpers();
		scope.carried = nullptr;
	}
	if (rgb_f32)
		delivery->carrier.copy(rgb_f32, ctx->staging_rgb.ptr, rgb_bytes);
	return ok();
}

rt_hip_status carried_frame::account(std::chrono::steady_clock::time_point entered, rt_hip_stats* stats)
{
	ctx->stats.readback_ms = end ? static_cast<float>(seconds_since(waited_from) * 1e3) : 0.0f;
	ctx->phases.host_issue_ms = static_cast<float>(std::chrono::duration<double>(issued - entered).count() * 1e3);
	ctx->phases.host_wait_ms = static_cast<float>(seconds_since(issued) * 1e3);
	if (end)
		ctx->phases.render_ms = elapsed_or_zero(ctx->render_begin, end);
	if (stats)
		return rt_hip_stats_fetch(ctx, stats);
	return ok();
}

rt_hip_status staged_results::deliver(frame_scope& scope, const void* d_packed, const void* d_rgb, const void* d_word, uint32_t* pixels_rgba8888, float* rgb_f32, uint32_t* out_word)
{
	unsigned char* const landing = staging.as<unsigned char>();
	const size_t word_at = rgba_bytes + rgb_bytes;
	hipError_t e = hipMemcpyAsync(landing, d_packed, rgba_bytes, hipMemcpyDeviceToHost, scope.stream);
	if (e == hipSuccess && rgb_bytes)
		e = hipMemcpyAsync(landing + rgba_bytes, d_rgb, rgb_bytes, hipMemcpyDeviceToHost, scope.stream);
	if (e == hipSuccess && word)
		e = hipMemcpyAsync(landing + word_at, d_word, words * sizeof(uint32_t), hipMemcpyDeviceToHost, scope.stream);
	waited_from = std::chrono::steady_clock::now();
	const hipError_t drained = scope.drain();
	RT_HIP_TRY(e);
	RT_HIP_TRY(drained);
	std::memcpy(pixels_rgba8888, landing, rgba_bytes);
	if (rgb_bytes)
		std::memcpy(rgb_f32, landing + rgba_bytes, rgb_bytes);
	if (word && out_word)
		std::memcpy(out_word, landing + word_at, words * sizeof(uint32_t));
	return ok();
}
}
