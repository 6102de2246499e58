// rt_amd/csrc/temporal.hip — temporal accumulation: the kernel that carries a history of accumulated samples across a
// camera move (reproject_frame), its device-level entry point rt_hip_reproject_device, and the drop-in rt_hip_render_temporal — one
// call, one frame: trace, guide, reproject against the context's history, optionally the a-trous filter, pack, deliver.
//
// A translation unit of its own: it changes nothing of the render kernels and uses the denoiser's guide and filter as they are
// (launch_guide, launch_filter of denoise.hip).  What a pixel of the step is — the projection, the taps, what makes a tap count, the
// blend — is reproject_rules.hpp's, the text the CPU restatement (tests/native/reproject_reference.cpp) runs too; here is only how
// the pixel's inputs reach the rule.
#include "internal.hpp"
#include "centre_ray.hpp"
#include "denoise.hpp"
#include "temporal.hpp"

namespace rt_hip
{
namespace reproject
{
	namespace leaf // the contract's own leaf functions, handed to the rule (reproject_rules.hpp has the list)
	{
		__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) { return rt_hip::dot({ ax, ay, az }, { bx, by, bz }); }
		__device__ __forceinline__ float fma(float a, float b, float c) { return rt_hip::fma(a, b, c); }
		__device__ __forceinline__ bool is_finite(float f) { return (__float_as_uint(f) & 0x7F800000u) != 0x7F800000u; }
	}
}
}
#include "reproject_rules.hpp"

#include <algorithm>
#include <exception>

namespace rt_hip
{
namespace
{
	// ---- reproject_frame: one lane per pixel ------------------------------------------------------------------------------------
	// A workgroup is a tile of 32 x 8 pixels, a wave two rows of 32 (as in atrous_pass): the pixel's own guide, colour and outputs are
	// row-contiguous, records move as 16-byte float4s.  The four taps' addresses depend on the data — where the surface point was in
	// the previous frame — so nothing is staged in LDS: neighbouring lanes project to neighbouring history pixels under any smooth
	// move, and their taps meet in L2.  The pixels that found history are counted per wave with a popcount of the ballot; one lane per
	// wave adds it to a word in HBM with an ordinary atomicAdd.
	constexpr uint32_t tile_w = 32, tile_h = 8;
	static_assert(tile_w * tile_h == block_threads, "one lane per pixel of the tile");

	struct projection
	{
		float m[16];
	};

	__global__ __launch_bounds__(block_threads) void reproject_frame(const frame_params p, const projection previous, const reproject::constants k, const float samples_in, const float4* __restrict__ guide,
																	   const float* __restrict__ rgb_in, const float* __restrict__ prev_rgb, const float4* __restrict__ prev_record, float* __restrict__ rgb_out,
																	   float4* __restrict__ record_out, uint32_t* __restrict__ found)
	{
		const uint32_t x = blockIdx.x * tile_w + (threadIdx.x & 31u), y = blockIdx.y * tile_h + (threadIdx.x >> 5);
		const bool alive = x < p.width && y < p.height;
		bool had_history = false;
		if (alive)
		{
			const int32_t width = static_cast<int32_t>(p.width), height = static_cast<int32_t>(p.height);
			const size_t pixel = static_cast<size_t>(y) * p.width + x;
			vec3 origin, dir;
			centre_ray(p, static_cast<float>(x), static_cast<float>(y), origin, dir);
			const float4 a = guide[pixel * 2u], b = guide[pixel * 2u + 1u];
			const reproject::rgb c = { rgb_in[pixel * 3u], rgb_in[pixel * 3u + 1u], rgb_in[pixel * 3u + 2u] };
			const reproject::result r = reproject::reproject_pixel(width, height, { a.x, a.y, a.z, a.w, __float_as_uint(b.w) }, c, samples_in, { origin.x, origin.y, origin.z, dir.x, dir.y, dir.z }, previous.m, prev_rgb != nullptr, k,
																   [&](int32_t qx, int32_t qy) -> reproject::tap
																   {
																	   // (the rule asks only for 0 <= qx < width, 0 <= qy < height)
																	   const size_t q = static_cast<size_t>(qy) * static_cast<size_t>(width) + static_cast<size_t>(qx);
																	   const float4 ra = prev_record[q * 2u], rb = prev_record[q * 2u + 1u];
																	   return { { ra.x, ra.y, ra.z, ra.w, rb.x, rb.y, rb.z, __float_as_uint(rb.w) }, { prev_rgb[q * 3u], prev_rgb[q * 3u + 1u], prev_rgb[q * 3u + 2u] } };
																   });
			rgb_out[pixel * 3u] = r.out.r;
			rgb_out[pixel * 3u + 1u] = r.out.g;
			rgb_out[pixel * 3u + 2u] = r.out.b;
			record_out[pixel * 2u] = make_float4(r.rec.px, r.rec.py, r.rec.pz, r.rec.length);
			record_out[pixel * 2u + 1u] = make_float4(r.rec.nx, r.rec.ny, r.rec.nz, __uint_as_float(r.rec.id));
			had_history = r.had_history;
		}
		const unsigned long long with_history = __ballot(had_history); // (every lane of the wave is here)
		if (found && (threadIdx.x & 63u) == 0u && with_history)
			atomicAdd(found, static_cast<uint32_t>(__popcll(with_history)));
	}

	// one step on device buffers (everything checked by the caller; ctx->device is current): the current camera is `matrix`
	rt_hip_status launch_reproject(uint32_t width, uint32_t height, const float* matrix, const float* previous_forward, const float* d_guide, const float* d_rgb_in, uint32_t samples_in, const float* d_prev_rgb,
								   const float* d_prev_record, const rt_hip_temporal_params& params, float* d_rgb_out, float* d_record_out, uint32_t* d_found, hipStream_t stream)
	{
		const frame_params f = centre_frame_params(width, height, matrix);
		projection previous{};
		if (d_prev_rgb)
			std::copy(previous_forward, previous_forward + 16, previous.m);
		if (d_found)
			RT_HIP_TRY(hipMemsetAsync(d_found, 0, sizeof(uint32_t), stream));
		const dim3 grid((width + tile_w - 1u) / tile_w, (height + tile_h - 1u) / tile_h);
		hipLaunchKernelGGL(reproject_frame, grid, dim3(block_threads), 0, stream, f, previous, reproject::constants_of(params), static_cast<float>(samples_in), reinterpret_cast<const float4*>(d_guide), d_rgb_in, d_prev_rgb,
						   reinterpret_cast<const float4*>(d_prev_record), d_rgb_out, reinterpret_cast<float4*>(d_record_out), d_found);
		RT_HIP_TRY(hipGetLastError());
		return ok();
	}

	// `params`, or the defaults; refused with the field's name
	rt_hip_status resolve_temporal(const char* who, const rt_hip_temporal_params* params, rt_hip_temporal_params& out)
	{
		out = params ? *params : default_temporal_params();
		const temporal_check checked = check_temporal_params(out);
		if (checked.status)
			return fail(checked.status, "%s: %s", who, checked.message);
		return ok();
	}
}
}

using namespace rt_hip;

extern "C" rt_hip_status rt_hip_temporal_default_params(rt_hip_temporal_params* out_params)
{
	if (!out_params)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_temporal_default_params: NULL argument");
	*out_params = default_temporal_params();
	return ok();
}

extern "C" rt_hip_status rt_hip_reproject_device(rt_hip_ctx* ctx,
												 uint32_t width,
												 uint32_t height,
												 const float prev_inverse_view_projection[16],
												 const float* d_guide,
												 const float* d_rgb_in,
												 uint32_t samples_in,
												 const float* d_prev_rgb,
												 const float* d_prev_record,
												 const rt_hip_temporal_params* params,
												 float* d_rgb_out,
												 float* d_record_out,
												 uint32_t* d_pixels_with_history,
												 void* stream)
{
	rt_hip_temporal_params p; // (what is wrong with the parameters is said before the context is looked at)
	if (const rt_hip_status st = resolve_temporal("rt_hip_reproject_device", params, p))
		return st;
	if (!ctx || !d_guide || !d_rgb_in || !d_rgb_out || !d_record_out)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_reproject_device: NULL argument");
	if ((d_prev_rgb == nullptr) != (d_prev_record == nullptr))
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_reproject_device: d_prev_rgb and d_prev_record are given together, or both NULL (no history)");
	if (d_prev_rgb && !prev_inverse_view_projection)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_reproject_device: NULL argument (a history without the matrix it was made under)");
	if (!width || !height || width > max_frame_side || height > max_frame_side)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_reproject_device: frame %ux%u (1 .. %u a side)", width, height, max_frame_side);
	if (!samples_in || samples_in > reproject::max_samples_in)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_reproject_device: samples_in = %u (1 .. %u)", samples_in, reproject::max_samples_in);
	if (reinterpret_cast<uintptr_t>(d_guide) % 16u || reinterpret_cast<uintptr_t>(d_record_out) % 16u || reinterpret_cast<uintptr_t>(d_prev_record) % 16u)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_reproject_device: d_guide, d_prev_record or d_record_out is not 16-byte aligned (two float4s per pixel)");
	const size_t pixels = static_cast<size_t>(width) * height;
	const size_t rgb_bytes = pixels * 3u * sizeof(float), record_bytes = pixels * reproject::record_words * sizeof(float);
	if (const rt_hip_status st = refuse_overlaps("rt_hip_reproject_device", { { d_rgb_out, rgb_bytes, "d_rgb_out" }, { d_record_out, record_bytes, "d_record_out" }, { d_pixels_with_history, sizeof(uint32_t), "d_pixels_with_history" } },
												 { { d_guide, record_bytes, "d_guide" }, { d_rgb_in, rgb_bytes, "d_rgb_in" }, { d_prev_rgb, rgb_bytes, "d_prev_rgb" }, { d_prev_record, record_bytes, "d_prev_record" } },
												 "a pixel reads other pixels' history", "the outputs overlap one another"))
		return st;
	float forward[16] = {};
	if (d_prev_rgb)
	{
		const temporal_check inverted = forward_view_projection(prev_inverse_view_projection, forward);
		if (inverted.status)
			return fail(inverted.status, "rt_hip_reproject_device: prev_inverse_view_projection: %s", inverted.message);
	}
	if (!ctx->have_scene)
		return fail(RT_HIP_NO_SCENE, "rt_hip_reproject_device: no scene uploaded");
	try
	{
		RT_HIP_TRY(hipSetDevice(ctx->device)); // (a multi-GPU, rank or frame-group context: the root member, like the other device-level calls)
		return launch_reproject(width, height, ctx->inverse_view_projection, forward, d_guide, d_rgb_in, samples_in, d_prev_rgb, d_prev_record, p, d_rgb_out, d_record_out, d_pixels_with_history, static_cast<hipStream_t>(stream));
	}
	catch (const std::exception& e)
	{
		return fail(RT_HIP_RUNTIME_ERROR, "rt_hip_reproject_device: %s", e.what());
	}
}

extern "C" rt_hip_status rt_hip_render_temporal(rt_hip_ctx* ctx,
												const rt_hip_scene* scene,
												uint32_t* pixels_rgba8888,
												uint32_t width,
												uint32_t height,
												uint64_t seed,
												uint32_t flags,
												const rt_hip_temporal_params* temporal,
												const rt_hip_denoise_params* filter,
												float* rgb_f32,
												rt_hip_stats* stats,
												rt_hip_temporal_info* out_info)
{
	rt_hip_temporal_params p; // (said before the context is looked at)
	if (const rt_hip_status st = resolve_temporal("rt_hip_render_temporal", temporal, p))
		return st;
	rt_hip_denoise_params spatial{};
	spatial.iterations = 0u; // no filter: the blended mean is packed as it is
	if (filter)
	{
		const denoise_check checked = check_denoise_params(*filter);
		if (checked.status)
			return fail(checked.status, "rt_hip_render_temporal: %s", checked.message);
		spatial = *filter;
	}
	if (!ctx || !scene || !pixels_rgba8888)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_render_temporal: NULL argument");
	if (!width || !height || width > max_frame_side || height > max_frame_side)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_render_temporal: frame %ux%u (1 .. %u a side)", width, height, max_frame_side);
	if (const rt_hip_status st = single_context_only("rt_hip_render_temporal", ctx))
		return st;
	if (const char* const refused = refused_guide_flag(flags))
		return fail(RT_HIP_UNSUPPORTED, "rt_hip_render_temporal: %s is not available for temporal frames (0x%x): they take RT_HIP_FLAG_SM_MATERIALS, RT_HIP_FLAG_BVH, RT_HIP_FLAG_BVH_DEVICE_BUILD, RT_HIP_FLAG_TRACE_BOXES and RT_HIP_FLAG_STATS", refused, flags);
	if (!scene->samples_per_pixel || scene->samples_per_pixel > reproject::max_samples_in)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_render_temporal: %u samples per pixel (1 .. %u a frame)", scene->samples_per_pixel, reproject::max_samples_in);
	const size_t pixels = static_cast<size_t>(width) * height;
	const size_t rgb_bytes = pixels * 3u * sizeof(float), rgba_bytes = pixels * sizeof(uint32_t), record_bytes = pixels * reproject::record_words * sizeof(float);
	const bool keep_stats = stats || (flags & RT_HIP_FLAG_STATS);
	try
	{
		RT_HIP_TRY(hipSetDevice(ctx->device));
		scene_request request;
		if (const rt_hip_status st = resident_scene(ctx, scene, request))
			return st;
		bool trace_boxes = false;
		if (const rt_hip_status st = guide_boxes("rt_hip_render_temporal", ctx, flags, &trace_boxes))
			return st;

		// is the context's history this frame's?
		temporal_state& t = ctx->temporal;
		const frame_key key = frame_key_of(request, scene, width, height, seed, flags & history_frame_flags);
		float forward[16] = {};
		bool carried = t.have_history && same_history(t.key, key) && t.rgb[t.current].bytes >= rgb_bytes && t.record[t.current].bytes >= record_bytes;
		if (carried && forward_view_projection(t.key.inverse_view_projection, forward).status) // (a matrix no frame could have been traced under)
			carried = false;
		const uint32_t from = t.current, to = t.current ^ 1u;
		t.have_history = false; // a frame that fails leaves the sets in an unknown state: no history from here until it has succeeded
		if (!carried)
			t.frames = 0;

		const hipStream_t s = ctx->stream;
		if (!t.end)
			RT_HIP_TRY(hipEventCreate(&t.end));
		for (uint32_t set = 0; set < 2u; set++)
			if (set == to || !carried) // (growing the set a carried history lives in is never needed: its size is part of the key)
			{
				RT_HIP_TRY(t.rgb[set].reserve(rgb_bytes));
				RT_HIP_TRY(t.record[set].reserve(record_bytes));
			}
		RT_HIP_TRY(t.traced.reserve(rgb_bytes));
		RT_HIP_TRY(t.guide.reserve(record_bytes));
		RT_HIP_TRY(t.packed.reserve(rgba_bytes));
		RT_HIP_TRY(t.found.reserve(sizeof(uint32_t)));
		if (rgb_f32 && spatial.iterations)
			RT_HIP_TRY(t.filtered.reserve(rgb_bytes));
		staged_results results{ t.staging, rgba_bytes, rgb_f32 ? rgb_bytes : 0u, true };
		RT_HIP_TRY(results.reserve());

		frame_scope scope(s, true); // whatever was enqueued has finished before anything returns
		// 1. the one-shot frame, by the launch rt_hip_render_device makes (its packed pixels land in `packed` and are overwritten below)
		if (const rt_hip_status st = render_device(ctx, width, height, seed, flags & render_flag_mask, nullptr, t.packed.as<uint32_t>(), t.traced.as<float>(), s, false, keep_stats, false))
			return st;
		// 2. its guide  3. the blend with the history  4. the spatial filter, or only the pack
		if (const rt_hip_status st = launch_guide(ctx, width, height, ctx->inverse_view_projection, trace_boxes, t.guide.as<float>(), s))
			return st;
		if (const rt_hip_status st = launch_reproject(width, height, ctx->inverse_view_projection, forward, t.guide.as<float>(), t.traced.as<float>(), scene->samples_per_pixel, carried ? t.rgb[from].as<float>() : nullptr,
													  carried ? t.record[from].as<float>() : nullptr, p, t.rgb[to].as<float>(), t.record[to].as<float>(), t.found.as<uint32_t>(), s))
			return st;
		const float* delivered = t.rgb[to].as<float>();
		if (const rt_hip_status st = launch_filter(ctx, width, height, t.rgb[to].as<float>(), t.guide.as<float>(), spatial, (rgb_f32 && spatial.iterations) ? t.filtered.as<float>() : nullptr, t.packed.as<uint32_t>(), s))
			return st;
		if (rgb_f32 && spatial.iterations)
			delivered = t.filtered.as<float>();
		if (keep_stats)
			RT_HIP_TRY(hipEventRecord(t.end, s));
		uint32_t found = 0;
		if (const rt_hip_status st = results.deliver(scope, t.packed.ptr, delivered, t.found.ptr, pixels_rgba8888, rgb_f32, &found))
			return st;
		t.current = to;
		t.key = key;
		t.have_history = true;
		t.frames++;
		if (out_info)
			*out_info = { t.frames, carried ? 0u : 1u, found, static_cast<uint32_t>(pixels) };
		ctx->stats.readback_ms = keep_stats ? static_cast<float>(seconds_since(results.waited_from) * 1e3) : 0.0f;
		if (stats)
		{
			if (const rt_hip_status st = rt_hip_stats_fetch(ctx, stats))
				return st;
			stats->render_ms = elapsed_or_zero(ctx->render_begin, t.end); // the traced frame and what follows it on the device
		}
		return ok();
	}
	catch (const std::exception& e) // nothing may propagate through the C boundary
	{
		return fail(RT_HIP_RUNTIME_ERROR, "rt_hip_render_temporal: %s", e.what());
	}
}
