// rt_amd/csrc/upsample.hip — guided upsampling: the kernel that rebuilds a full-size frame from a traced low one
// (upsample_frame), its device-level entry point rt_hip_upsample_device, the two host-only helpers of include/rt_hip.h, and the
// drop-in rt_hip_render_upscaled — one call, one frame: trace low, build both guides, optionally filter the low mean, rebuild.
//
// A translation unit of its own: it changes nothing of the render kernels and launches the frame, the guide and the filter through
// what render.hip and denoise.hip already offer (render_device, launch_guide, launch_filter).  What a pixel of the reconstruction is
// — the geometry, the weights, the order of the adds, the orphan rule — is upsample_rules.hpp's, the text the CPU restatement
// (tests/native/upsample_reference.cpp) runs too; here is only how a low tap reaches the rule.
#include "internal.hpp"
#include "denoise.hpp"
#include "upsample.hpp"

namespace rt_hip
{
namespace denoise
{
	namespace leaf // the contract's own leaf functions, handed to the rules (denoise_rules.hpp has the list)
	{
		__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) { return rt_hip::dot({ ax, ay, az }, { bx, by, bz }); }
		__device__ __forceinline__ float sqrt_rn(float x) { return rt_hip::sqrt_rn(x); }
		__device__ __forceinline__ uint32_t pack(float r, float g, float b) { return rt_hip::pack_rgba8888({ r, g, b }); }
	}
}
}
#include "upsample_rules.hpp"

#include <exception>

namespace rt_hip
{
namespace
{
	// ---- upsample_frame: one lane per FULL pixel, 16 x 16 workgroups (four waves of 4 rows) -----------------------------------------
	// A full pixel reads four low taps of 44 bytes, and its neighbours read the same ones: at factor 2 the 256 pixels of a workgroup
	// share about 100 low pixels.  The workgroup therefore stages, once, every low tap its block can reach — from the smallest X0 / Y0
	// to the largest X1 / Y1 of the block's pixels inside the frame, by the geometry rule itself (source_of), clipped to the low frame
	// — into LDS: at most 17 x 17 records (w == W; 15 w / W + 2 otherwise) of 11 words, 8 of guide and 3 of colour.  The records lie
	// one behind the other, 11 words apart: an odd stride, so the lanes of a row, which read the SAME word of neighbouring records,
	// fall on different banks, and lanes that share a tap are served by one broadcast.  Memory sees each staged record once (two
	// 16-byte loads and three words), each full pixel's own guide as two 16-byte loads, and the stores: about 48 bytes per full pixel
	// plus 44 / factor^2.  A lane outside the frame stages and waits at the barrier like the others and stores nothing.
	// The orphans: one ballot and popcount per wave, one integer atomic add per wave that has any.
	constexpr uint32_t tile = 16;
	static_assert(tile * tile == block_threads, "one lane per full pixel of the block");
	constexpr int32_t staged_side = upsample::max_staged_side;

	__global__ __launch_bounds__(block_threads) void upsample_frame(const uint32_t W, const uint32_t H, const uint32_t w, const uint32_t h, const uint32_t blocks_x, const rt_hip_upsample_params params,
																	 const float* __restrict__ low, const float4* __restrict__ guide_low, const float4* __restrict__ guide_full, float* __restrict__ dst,
																	 uint32_t* __restrict__ rgba, uint32_t* __restrict__ orphans)
	{
		__shared__ float staged[staged_side * staged_side * upsample::low_words];
		const upsample::constants k = upsample::constants_of(params);
		const uint32_t block_y = blockIdx.x / blocks_x, block_x = blockIdx.x - block_y * blocks_x; // (wave-uniform)
		const uint32_t x0 = block_x * tile, y0 = block_y * tile;								   // (inside the frame: the grid is cut from it)
		const uint32_t x_last = min(x0 + tile - 1u, W - 1u), y_last = min(y0 + tile - 1u, H - 1u);
		const int32_t lo_x = max(upsample::source_of(x0, W, w).first, 0), hi_x = min(upsample::source_of(x_last, W, w).first + 1, static_cast<int32_t>(w) - 1);
		const int32_t lo_y = max(upsample::source_of(y0, H, h).first, 0), hi_y = min(upsample::source_of(y_last, H, h).first + 1, static_cast<int32_t>(h) - 1);
		const int32_t span_x = min(hi_x - lo_x + 1, staged_side), span_y = min(hi_y - lo_y + 1, staged_side); // (1 .. 17 by the rule; the clamp keeps LDS writes in bounds whatever happens)
		for (int32_t slot = static_cast<int32_t>(threadIdx.x); slot < span_x * span_y; slot += static_cast<int32_t>(block_threads))
		{
			const int32_t qy = lo_y + slot / span_x, qx = lo_x + slot % span_x; // (inside the low frame by the clip)
			const size_t pixel = static_cast<size_t>(qy) * static_cast<size_t>(w) + static_cast<size_t>(qx);
			const float4 a = guide_low[pixel * 2u], b = guide_low[pixel * 2u + 1u];
			float* const record = staged + slot * static_cast<int32_t>(upsample::low_words);
			record[0] = a.x, record[1] = a.y, record[2] = a.z, record[3] = a.w;
			record[4] = b.x, record[5] = b.y, record[6] = b.z, record[7] = b.w;
			record[8] = low[pixel * 3u], record[9] = low[pixel * 3u + 1u], record[10] = low[pixel * 3u + 2u];
		}
		__syncthreads();

		const uint32_t x = x0 + (threadIdx.x & (tile - 1u)), y = y0 + threadIdx.x / tile;
		const bool alive = x < W && y < H;
		bool orphan = false;
		if (alive)
		{
			const size_t pixel = static_cast<size_t>(y) * static_cast<size_t>(W) + static_cast<size_t>(x);
			const float4 a = guide_full[pixel * 2u], b = guide_full[pixel * 2u + 1u];
			const denoise::guide p = { a.x, a.y, a.z, a.w, b.x, b.y, b.z, __float_as_uint(b.w) };
			const upsample::pixel out = upsample::upsample_pixel(x, y, W, H, w, h, k,
																 [&](int32_t qx, int32_t qy) -> denoise::tap
																 {
																	 // lo <= q <= hi: q is one of this pixel's taps inside the low frame, and the block's span holds them all
																	 const float* const r = staged + ((qy - lo_y) * span_x + (qx - lo_x)) * static_cast<int32_t>(upsample::low_words);
																	 return { { r[0], r[1], r[2], r[3], r[4], r[5], r[6], __float_as_uint(r[7]) }, { r[8], r[9], r[10] } };
																 },
																 p);
			orphan = out.orphan;
			if (dst)
			{
				dst[pixel * 3u] = out.c.r;
				dst[pixel * 3u + 1u] = out.c.g;
				dst[pixel * 3u + 2u] = out.c.b;
			}
			if (rgba)
				rgba[pixel] = denoise::finish(out.c);
		}
		if (orphans) // (wave-uniform)
		{
			const uint32_t here = static_cast<uint32_t>(__popcll(__ballot(orphan)));
			if (here && (threadIdx.x & 63u) == 0u)
				atomicAdd(orphans, here);
		}
	}

	// `params`, or the defaults; refused with the field's name
	rt_hip_status resolve_upsample(const char* who, const rt_hip_upsample_params* params, rt_hip_upsample_params& out)
	{
		out = params ? *params : default_upsample_params();
		const upsample_check checked = check_upsample_params(out);
		if (checked.status)
			return fail(checked.status, "%s: %s", who, checked.message);
		return ok();
	}

	// the reconstruction on device buffers (everything checked by the caller; the context's device is current)
	rt_hip_status launch_upsample(const char* who, uint32_t W, uint32_t H, uint32_t w, uint32_t h, const float* d_low, const float* d_guide_low, const float* d_guide_full, const rt_hip_upsample_params& params, float* d_out,
								  uint32_t* d_rgba, uint32_t* d_orphans, hipStream_t stream)
	{
		const uint64_t blocks_x = (W + tile - 1u) / tile, blocks_y = (H + tile - 1u) / tile;
		if (blocks_x * blocks_y > 0x7FFFFFFFull)
			return fail(RT_HIP_INVALID_ARGUMENT, "%s: frame %ux%u is more than 2^31 - 1 blocks of %u x %u pixels", who, W, H, tile, tile);
		if (d_orphans)
			RT_HIP_TRY(hipMemsetAsync(d_orphans, 0, sizeof(uint32_t), stream));
		hipLaunchKernelGGL(upsample_frame, dim3(static_cast<uint32_t>(blocks_x * blocks_y)), dim3(block_threads), 0, stream, W, H, w, h, static_cast<uint32_t>(blocks_x), params, d_low,
						   reinterpret_cast<const float4*>(d_guide_low), reinterpret_cast<const float4*>(d_guide_full), d_out, d_rgba, d_orphans);
		RT_HIP_TRY(hipGetLastError());
		return ok();
	}
}
}

using namespace rt_hip;

extern "C" rt_hip_status rt_hip_upsample_default_params(rt_hip_upsample_params* out_params)
{
	if (!out_params)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_upsample_default_params: NULL argument");
	*out_params = default_upsample_params();
	return ok();
}

extern "C" rt_hip_status rt_hip_upsample_low_size(uint32_t width, uint32_t height, uint32_t factor, uint32_t* out_low_width, uint32_t* out_low_height)
{
	const upsample_check checked = upsample_low_size(width, height, factor, out_low_width, out_low_height);
	if (checked.status)
		return fail(checked.status, "rt_hip_upsample_low_size: %s", checked.message);
	return ok();
}

extern "C" rt_hip_status rt_hip_upsample_device(rt_hip_ctx* ctx,
												uint32_t width,
												uint32_t height,
												uint32_t low_width,
												uint32_t low_height,
												const float* d_rgb_low,
												const float* d_guide_low,
												const float* d_guide_full,
												const rt_hip_upsample_params* params,
												float* d_rgb_out,
												uint32_t* d_rgba8_out,
												uint32_t* d_orphans,
												void* stream)
{
	rt_hip_upsample_params p; // (what is wrong with the parameters is said before the context is looked at)
	if (const rt_hip_status st = resolve_upsample("rt_hip_upsample_device", params, p))
		return st;
	if (!ctx || !d_rgb_low || !d_guide_low || !d_guide_full)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_upsample_device: NULL argument");
	if (!d_rgb_out && !d_rgba8_out)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_upsample_device: NULL argument (d_rgb_out and d_rgba8_out are both NULL: nothing to write)");
	if (const upsample_check sizes = check_upsample_sizes(width, height, low_width, low_height); sizes.status)
		return fail(sizes.status, "rt_hip_upsample_device: %s", sizes.message);
	if (reinterpret_cast<uintptr_t>(d_guide_low) % 16u || reinterpret_cast<uintptr_t>(d_guide_full) % 16u)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_upsample_device: d_guide_low or d_guide_full is not 16-byte aligned (two float4s per pixel)");
	const size_t pixels = static_cast<size_t>(width) * height, low_pixels = static_cast<size_t>(low_width) * low_height;
	if (const rt_hip_status st = refuse_overlaps("rt_hip_upsample_device", { { d_rgb_out, pixels * 3u * sizeof(float), "d_rgb_out" }, { d_rgba8_out, pixels * sizeof(uint32_t), "d_rgba8_out" }, { d_orphans, sizeof(uint32_t), "d_orphans" } },
												 { { d_rgb_low, low_pixels * 3u * sizeof(float), "d_rgb_low" }, { d_guide_low, low_pixels * denoise::guide_words * sizeof(float), "d_guide_low" }, { d_guide_full, pixels * denoise::guide_words * sizeof(float), "d_guide_full" } },
												 "a pixel reads other pixels' taps"))
		return st;
	try
	{
		RT_HIP_TRY(hipSetDevice(ctx->device)); // (a multi-GPU, rank or frame-group context: the root member, like the other device-level calls)
		return launch_upsample("rt_hip_upsample_device", width, height, low_width, low_height, d_rgb_low, d_guide_low, d_guide_full, p, d_rgb_out, d_rgba8_out, d_orphans, static_cast<hipStream_t>(stream));
	}
	catch (const std::exception& e)
	{
		return fail(RT_HIP_RUNTIME_ERROR, "rt_hip_upsample_device: %s", e.what());
	}
}

extern "C" rt_hip_status rt_hip_render_upscaled(rt_hip_ctx* ctx,
												const rt_hip_scene* scene,
												uint32_t* pixels_rgba8888,
												uint32_t width,
												uint32_t height,
												uint64_t seed,
												uint32_t flags,
												uint32_t factor,
												const rt_hip_upsample_params* upsample_params,
												const rt_hip_denoise_params* filter,
												float* rgb_f32,
												rt_hip_stats* stats,
												rt_hip_upscale_info* out_info)
{
	rt_hip_upsample_params p; // (said before the context is looked at)
	if (const rt_hip_status st = resolve_upsample("rt_hip_render_upscaled", upsample_params, p))
		return st;
	if (filter)
	{
		const denoise_check checked = check_denoise_params(*filter);
		if (checked.status)
			return fail(checked.status, "rt_hip_render_upscaled: %s", checked.message);
	}
	if (!ctx || !scene || !pixels_rgba8888)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_render_upscaled: NULL argument");
	if (!width || !height || width > max_frame_side || height > max_frame_side)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_render_upscaled: frame %ux%u (1 .. %u a side)", width, height, max_frame_side);
	if (factor < 2u || factor > upsample::max_factor)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_render_upscaled: factor = %u (2 .. %u)", factor, upsample::max_factor);
	if (const rt_hip_status st = single_context_only("rt_hip_render_upscaled", ctx))
		return st;
	if (const char* const refused = refused_guide_flag(flags))
		return fail(RT_HIP_UNSUPPORTED, "rt_hip_render_upscaled: %s is not available for upscaled frames (0x%x): they take RT_HIP_FLAG_SM_MATERIALS, RT_HIP_FLAG_BVH, RT_HIP_FLAG_BVH_DEVICE_BUILD, RT_HIP_FLAG_TRACE_BOXES and RT_HIP_FLAG_STATS", refused, flags);
	uint32_t w = 0, h = 0;
	if (const upsample_check low = upsample_low_size(width, height, factor, &w, &h); low.status)
		return fail(low.status, "rt_hip_render_upscaled: %s", low.message);
	const size_t pixels = static_cast<size_t>(width) * height, low_pixels = static_cast<size_t>(w) * h;
	const size_t rgb_bytes = pixels * 3u * sizeof(float), rgba_bytes = pixels * sizeof(uint32_t);
	const size_t low_rgb_bytes = low_pixels * 3u * sizeof(float);
	const bool keep_stats = stats || (flags & RT_HIP_FLAG_STATS);
	try
	{
		RT_HIP_TRY(hipSetDevice(ctx->device));
		scene_request request;
		if (const rt_hip_status st = resident_scene(ctx, scene, request))
			return st;
		bool trace_boxes = false;
		if (const rt_hip_status st = guide_boxes("rt_hip_render_upscaled", ctx, flags, &trace_boxes))
			return st;

		upscale_state& u = ctx->upscale;
		const hipStream_t s = ctx->stream;
		if (!u.end)
			RT_HIP_TRY(hipEventCreate(&u.end));
		RT_HIP_TRY(u.low_mean.reserve(low_rgb_bytes));
		RT_HIP_TRY(u.low_packed.reserve(low_pixels * sizeof(uint32_t)));
		if (filter)
			RT_HIP_TRY(u.low_filtered.reserve(low_rgb_bytes));
		RT_HIP_TRY(u.guide_low.reserve(low_pixels * denoise::guide_words * sizeof(float)));
		RT_HIP_TRY(u.guide_full.reserve(pixels * denoise::guide_words * sizeof(float)));
		if (rgb_f32)
			RT_HIP_TRY(u.rgb.reserve(rgb_bytes));
		RT_HIP_TRY(u.packed.reserve(rgba_bytes));
		RT_HIP_TRY(u.orphans.reserve(sizeof(uint32_t)));
		staged_results results{ u.staging, rgba_bytes, rgb_f32 ? rgb_bytes : 0u, true };
		RT_HIP_TRY(results.reserve());

		frame_scope scope(s, true); // whatever was enqueued has finished before anything returns
		// 1. the one-shot LOW frame, by the launch rt_hip_render_device makes (its packed pixels are not used)
		if (const rt_hip_status st = render_device(ctx, w, h, seed, flags & render_flag_mask, nullptr, u.low_packed.as<uint32_t>(), u.low_mean.as<float>(), s, false, keep_stats, false))
			return st;
		// 2. the guide at both sizes  3. the filter on the low mean  4. the reconstruction
		if (const rt_hip_status st = launch_guide(ctx, w, h, ctx->inverse_view_projection, trace_boxes, u.guide_low.as<float>(), s))
			return st;
		if (const rt_hip_status st = launch_guide(ctx, width, height, ctx->inverse_view_projection, trace_boxes, u.guide_full.as<float>(), s))
			return st;
		const float* low = u.low_mean.as<float>();
		if (filter)
		{
			if (const rt_hip_status st = launch_filter(ctx, w, h, u.low_mean.as<float>(), u.guide_low.as<float>(), *filter, u.low_filtered.as<float>(), nullptr, s))
				return st;
			low = u.low_filtered.as<float>();
		}
		if (const rt_hip_status st = launch_upsample("rt_hip_render_upscaled", width, height, w, h, low, u.guide_low.as<float>(), u.guide_full.as<float>(), p, rgb_f32 ? u.rgb.as<float>() : nullptr, u.packed.as<uint32_t>(), u.orphans.as<uint32_t>(), s))
			return st;
		if (keep_stats)
			RT_HIP_TRY(hipEventRecord(u.end, s));
		uint32_t orphans = 0;
		if (const rt_hip_status st = results.deliver(scope, u.packed.ptr, u.rgb.ptr, u.orphans.ptr, pixels_rgba8888, rgb_f32, &orphans))
			return st;
		if (out_info)
			*out_info = { w, h, orphans, static_cast<uint32_t>(pixels) };
		ctx->stats.readback_ms = keep_stats ? static_cast<float>(seconds_since(results.waited_from) * 1e3) : 0.0f;
		if (stats)
		{
			if (const rt_hip_status st = rt_hip_stats_fetch(ctx, stats))
				return st;
			stats->render_ms = elapsed_or_zero(ctx->render_begin, u.end); // the traced low frame and what follows it on the device
		}
		return ok();
	}
	catch (const std::exception& e) // nothing may propagate through the C boundary
	{
		return fail(RT_HIP_RUNTIME_ERROR, "rt_hip_render_upscaled: %s", e.what());
	}
}
