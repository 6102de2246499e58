// rt_amd/csrc/denoise.hip — the guide-buffer denoiser for low-sample frames: the kernel that writes the first-hit
// guide of the resident scene (guide_frame), the edge-avoiding a-trous wavelet filter steered by it (atrous_pass, one launch per
// iteration), and the three entry points of include/rt_hip.h — rt_hip_guide_device, rt_hip_denoise_device and
// rt_hip_denoise_progressive, which applies both to the accumulation in flight of rt_hip_render_progressive without the float frame
// crossing the bus on its way in.
//
// A translation unit of its own: it INCLUDES the contract's headers (contract.hpp, scan.hpp) and changes nothing of the render
// kernels.  What a pixel of the filter is — the weights, the order of the adds, the finish — is denoise_rules.hpp's, the text the
// CPU restatement (tests/native/denoise_reference.cpp) runs too; here is only how a tap reaches the rule.
#include "internal.hpp"
#include "scan.hpp"
#include "denoise.hpp"
#include "centre_ray.hpp"

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
#include "denoise_rules.hpp"

#include <algorithm>
#include <exception>

namespace rt_hip
{
namespace
{
	// ---- guide_frame: one thread per pixel, the path tracer's sample-0 primary ray, one closest-hit query ----------------------
	// The ray is centre_ray.hpp's: the one the render kernels build for sample 0, through the pixel centre (reproject_frame of
	// temporal.hip builds the same one).
	// The query is the tracer's (scan.hpp): the 0.001 rule, ties to the lower index, select(spheres, planes) and — under
	// RT_HIP_FLAG_TRACE_BOXES only — select(boxes, ...).  A linear scan over the resident tables: every lane of a wave walks the same
	// primitive, so the reads are wave-uniform (scalar loads), as in the preview; one query per pixel needs no more.
	__global__ __launch_bounds__(block_threads) void guide_frame(const frame_params p, const device_scene s, const uint32_t trace_boxes, float4* __restrict__ out)
	{
		const uint32_t x = blockIdx.x * 64u + (threadIdx.x & 63u);
		const uint32_t y = blockIdx.y * (block_threads / 64u) + (threadIdx.x >> 6);
		const bool alive = x < p.width && y < p.height;
		const float fx = static_cast<float>(alive ? x : 0u), fy = static_cast<float>(alive ? y : 0u); // (a lane outside the frame traces pixel (0, 0) and stores nothing)
		vec3 origin, dir;
		centre_ray(p, fx, fy, origin, dir);

		candidate spheres = { 0.0f, 0u, false }, planes = { 0.0f, 0u, false }, boxes = { 0.0f, 0u, false };
		scan_lds<true>(spheres, origin, dir, s.primitive_geometry, s.n_spheres, 0u); // (any float4 table with wave-uniform addresses, not LDS only)
		scan_lds<false>(planes, origin, dir, s.primitive_geometry + s.n_spheres, s.n_planes, 0u);
		const vec3 inv = box_reciprocals(dir);
		if (trace_boxes) // (wave-uniform)
			scan_boxes(boxes, origin, inv, s.box_bounds, s.n_boxes);
		float distance;
		uint32_t index;
		const uint32_t kind = select_hit(spheres, planes, boxes, distance, index); // (without a box candidate: select(spheres, planes))
		vec3 normal = { 0.0f, 0.0f, 0.0f };
		float4 shading = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
		uint32_t scatter;
		fetch_hit<false>(s, s.box_bounds, origin, dir, inv, kind, distance, index, normal, shading, scatter);
		uint32_t id = 0u;
		if (kind)
			id = 1u + (kind == 1u ? index : (kind == 2u ? s.n_spheres + index : s.n_spheres + s.n_planes + index));
		else
		{
			const vec3 colour = sky(dir.y);
			normal = { 0.0f, 0.0f, 0.0f };
			shading = make_float4(colour.x, colour.y, colour.z, 0.0f);
		}
		if (alive)
		{
			const size_t o = (static_cast<size_t>(y) * p.width + x) * 2u;
			out[o] = make_float4(normal.x, normal.y, normal.z, distance);
			out[o + 1u] = make_float4(shading.x, shading.y, shading.z, __uint_as_float(id));
		}
	}

	// ---- atrous_pass: one iteration of the filter ------------------------------------------------------------------------------
	// Every pixel reads 25 taps of 12 bytes of colour and 32 bytes of guide.  For the first two iterations (taps 1 and 2 pixels apart)
	// the footprints of neighbouring pixels overlap almost entirely: a workgroup stages its tile of 32 x 8 pixels with a halo of
	// 2 * step into LDS once — three float4s per pixel (guide, guide, colour), so every LDS read is a 16-byte one and neighbouring
	// lanes read neighbouring slots — and all 25 taps come from there: 44 bytes per staged pixel from memory, where 25 taps apiece
	// would ask L2 for 1100.  From step 4 on a pixel's taps are 25 separate cache lines which no neighbour in the tile shares within
	// the iteration's reach of a tile's rows; the halo would be larger than the tile (step 4: 48 x 24 staged for 32 x 8 used), so those
	// iterations gather straight from L2 (STEP == 0: the step is a run-time value).
	// A lane is one pixel, a wave two rows of 32: row-contiguous loads and stores of 384 bytes.  The arithmetic and the order of the
	// adds are filter_pixel's: the template parameter changes where `fetch` reads, nothing else.
	constexpr int32_t tile_w = 32, tile_h = 8;
	static_assert(tile_w * tile_h == static_cast<int32_t>(block_threads), "one lane per pixel of the tile");

	template <int32_t STEP>
	__global__ __launch_bounds__(block_threads) void atrous_pass(const int32_t width, const int32_t height, const rt_hip_denoise_params params, const uint32_t iteration,
																  const float* __restrict__ src, const float4* __restrict__ guide, float* __restrict__ dst, uint32_t* __restrict__ rgba)
	{
		const denoise::pass_constants k = denoise::constants_of(params, iteration);
		const int32_t x0 = static_cast<int32_t>(blockIdx.x) * tile_w, y0 = static_cast<int32_t>(blockIdx.y) * tile_h;
		const int32_t x = x0 + static_cast<int32_t>(threadIdx.x & 31u), y = y0 + static_cast<int32_t>(threadIdx.x >> 5);
		const bool alive = x < width && y < height;
		denoise::rgb result = { 0.0f, 0.0f, 0.0f };
		if constexpr (STEP != 0)
		{
			constexpr int32_t halo = 2 * STEP, staged_w = tile_w + 2 * halo, staged_h = tile_h + 2 * halo;
			__shared__ float4 guide_a[staged_w * staged_h], guide_b[staged_w * staged_h], colour[staged_w * staged_h];
			for (int32_t slot = static_cast<int32_t>(threadIdx.x); slot < staged_w * staged_h; slot += static_cast<int32_t>(block_threads))
			{
				const int32_t qx = x0 - halo + slot % staged_w, qy = y0 - halo + slot / staged_w;
				if (qx >= 0 && qx < width && qy >= 0 && qy < height) // (slots outside the frame stay unwritten: the rule never fetches them)
				{
					const size_t pixel = static_cast<size_t>(qy) * static_cast<size_t>(width) + static_cast<size_t>(qx);
					guide_a[slot] = guide[pixel * 2u];
					guide_b[slot] = guide[pixel * 2u + 1u];
					colour[slot] = make_float4(src[pixel * 3u], src[pixel * 3u + 1u], src[pixel * 3u + 2u], 0.0f);
				}
			}
			__syncthreads();
			if (alive)
				result = denoise::filter_pixel(x, y, width, height, k,
											   [&](int32_t qx, int32_t qy) -> denoise::tap
											   {
												   // |qx - x| and |qy - y| are at most 2 * STEP = halo (k.step == STEP: the host picks the build by the iteration)
												   const int32_t slot = (qy - (y0 - halo)) * staged_w + (qx - (x0 - halo));
												   const float4 a = guide_a[slot], b = guide_b[slot], c = colour[slot];
												   return { { a.x, a.y, a.z, a.w, b.x, b.y, b.z, __float_as_uint(b.w) }, { c.x, c.y, c.z } };
											   });
		}
		else if (alive)
			result = denoise::filter_pixel(x, y, width, height, k,
										   [&](int32_t qx, int32_t qy) -> denoise::tap
										   {
											   const size_t pixel = static_cast<size_t>(qy) * static_cast<size_t>(width) + static_cast<size_t>(qx);
											   const float4 a = guide[pixel * 2u], b = guide[pixel * 2u + 1u];
											   return { { a.x, a.y, a.z, a.w, b.x, b.y, b.z, __float_as_uint(b.w) }, { src[pixel * 3u], src[pixel * 3u + 1u], src[pixel * 3u + 2u] } };
										   });
		if (alive)
		{
			const size_t pixel = static_cast<size_t>(y) * static_cast<size_t>(width) + static_cast<size_t>(x);
			if (dst)
			{
				dst[pixel * 3u] = result.r;
				dst[pixel * 3u + 1u] = result.g;
				dst[pixel * 3u + 2u] = result.b;
			}
			if (rgba)
				rgba[pixel] = denoise::finish(result);
		}
	}

	// iterations == 0: the image as it is, and its packed pixels
	__global__ __launch_bounds__(block_threads) void finish_frame(const size_t pixels, const float* __restrict__ src, float* __restrict__ dst, uint32_t* __restrict__ rgba)
	{
		const size_t pixel = static_cast<size_t>(blockIdx.x) * block_threads + threadIdx.x;
		if (pixel >= pixels)
			return;
		const denoise::rgb c = { src[pixel * 3u], src[pixel * 3u + 1u], src[pixel * 3u + 2u] };
		if (dst)
		{
			dst[pixel * 3u] = c.r;
			dst[pixel * 3u + 1u] = c.g;
			dst[pixel * 3u + 2u] = c.b;
		}
		if (rgba)
			rgba[pixel] = denoise::finish(c);
	}

	// the mean of an accumulation: accumulator / samples_done, the fold's own division (kernels.hip; correctly rounded)
	__global__ __launch_bounds__(block_threads) void mean_frame(const size_t words, const float* __restrict__ sums, const float n, float* __restrict__ mean)
	{
		const size_t i = static_cast<size_t>(blockIdx.x) * block_threads + threadIdx.x;
		if (i < words)
			mean[i] = sums[i] / n;
	}

	// `params`, or the defaults; refused with the field's name
	rt_hip_status resolve_params(const char* who, const rt_hip_denoise_params* params, rt_hip_denoise_params& out)
	{
		out = params ? *params : default_denoise_params();
		const denoise_check checked = check_denoise_params(out);
		if (checked.status)
			return fail(checked.status, "%s: %s", who, checked.message);
		return ok();
	}
} // namespace (this file's own: the kernels and resolve_params)

	// ---- the host helpers temporal.hip uses too: namespace rt_hip, declared in internal.hpp -------------------------------------------
	const char* refused_guide_flag(uint32_t flags)
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
						{ RT_HIP_FLAG_BOX_BVH, "RT_HIP_FLAG_BOX_BVH" }, // (the guide kernel keeps its linear scan over at most box_max_count boxes)
						{ RT_HIP_FLAG_EMISSION, "RT_HIP_FLAG_EMISSION" }, // (the guide's albedo knows no lights: temporal frames and the guide itself)
						{ RT_HIP_FLAG_DIRECT_LIGHT, "RT_HIP_FLAG_DIRECT_LIGHT" }, // (its modifier)
						{ RT_HIP_FLAG_THIN_LENS, "RT_HIP_FLAG_THIN_LENS" } };	  // (the guide is the pinhole's centre ray: temporal and upscaled frames, and the guide itself)
		for (const auto& flag : refused)
			if (flags & flag.bit)
				return flag.name;
		uint32_t known = pass_flag_mask | RT_HIP_FLAG_STATS | RT_HIP_FLAG_TRACE_BOXES;
		for (const auto& flag : refused)
			known |= flag.bit;
		return (flags & ~known) ? "unknown flag bits" : nullptr;
	}

	bool buffers_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes)
	{
		const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
		return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
	}

	// the constants centre_ray() reads for a whole width x height frame seen through `matrix`
	frame_params centre_frame_params(uint32_t width, uint32_t height, const float* matrix)
	{
		frame_request wanted{};
		wanted.width = width, wanted.height = height, wanted.partition = { 0u, 1u, RT_HIP_DEFAULT_STRIPE_ROWS };
		wanted.samples_per_pixel = 1u, wanted.max_bounces = 1u, wanted.seed = 0u, wanted.whole_frame_buffers = false; // (the centre ray draws nothing)
		std::copy(matrix, matrix + 16, wanted.inverse_view_projection);
		return make_frame_params(wanted);
	}

	// the guide of `ctx`'s resident scene seen through `matrix` (everything checked by the caller; ctx->device is current)
	rt_hip_status launch_guide(rt_hip_ctx* ctx, uint32_t width, uint32_t height, const float* matrix, bool trace_boxes, float* d_guide, hipStream_t stream)
	{
		const frame_params f = centre_frame_params(width, height, matrix);
		const dim3 grid((width + 63u) / 64u, (height + block_threads / 64u - 1u) / (block_threads / 64u));
		hipLaunchKernelGGL(guide_frame, grid, dim3(block_threads), 0, stream, f, ctx->scene, trace_boxes ? 1u : 0u, reinterpret_cast<float4*>(d_guide));
		RT_HIP_TRY(hipGetLastError());
		return ok();
	}

	// the filter on device buffers (everything checked by the caller; ctx->device is current)
	rt_hip_status launch_filter(rt_hip_ctx* ctx, uint32_t width, uint32_t height, const float* d_in, const float* d_guide, const rt_hip_denoise_params& params, float* d_out, uint32_t* d_rgba, hipStream_t stream)
	{
		const size_t pixels = static_cast<size_t>(width) * height;
		if (!params.iterations)
		{
			hipLaunchKernelGGL(finish_frame, dim3(static_cast<uint32_t>((pixels + block_threads - 1u) / block_threads)), dim3(block_threads), 0, stream, pixels, d_in, d_out, d_rgba);
			RT_HIP_TRY(hipGetLastError());
			return ok();
		}
		if (params.iterations > 1u)
			RT_HIP_TRY(ctx->denoise.scratch[0].reserve(pixels * 3u * sizeof(float)));
		if (params.iterations > 2u)
			RT_HIP_TRY(ctx->denoise.scratch[1].reserve(pixels * 3u * sizeof(float)));
		const dim3 grid((width + static_cast<uint32_t>(tile_w) - 1u) / static_cast<uint32_t>(tile_w), (height + static_cast<uint32_t>(tile_h) - 1u) / static_cast<uint32_t>(tile_h));
		const float4* const guide = reinterpret_cast<const float4*>(d_guide);
		const int32_t w = static_cast<int32_t>(width), h = static_cast<int32_t>(height);
		const float* from = d_in;
		for (uint32_t i = 0; i < params.iterations; i++)
		{
			const bool last = i + 1u == params.iterations;
			float* const to = last ? d_out : ctx->denoise.scratch[i & 1u].as<float>(); // (the last iteration writes the caller's image, or only packs)
			uint32_t* const packed = last ? d_rgba : nullptr;
			if (i == 0u)
				hipLaunchKernelGGL(atrous_pass<1>, grid, dim3(block_threads), 0, stream, w, h, params, i, from, guide, to, packed);
			else if (i == 1u)
				hipLaunchKernelGGL(atrous_pass<2>, grid, dim3(block_threads), 0, stream, w, h, params, i, from, guide, to, packed);
			else
				hipLaunchKernelGGL(atrous_pass<0>, grid, dim3(block_threads), 0, stream, w, h, params, i, from, guide, to, packed);
			RT_HIP_TRY(hipGetLastError());
			from = to;
		}
		return ok();
	}

} // namespace rt_hip

using namespace rt_hip;

extern "C" rt_hip_status rt_hip_denoise_default_params(rt_hip_denoise_params* out_params)
{
	if (!out_params)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_denoise_default_params: NULL argument");
	*out_params = default_denoise_params();
	return ok();
}

extern "C" rt_hip_status rt_hip_guide_device(rt_hip_ctx* ctx, uint32_t width, uint32_t height, uint32_t flags, float* d_guide, void* stream)
{
	if (!ctx || !d_guide)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_guide_device: NULL argument");
	if (!width || !height || width > max_frame_side || height > max_frame_side)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_guide_device: frame %ux%u (1 .. %u a side)", width, height, max_frame_side);
	if (reinterpret_cast<uintptr_t>(d_guide) % 16u)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_guide_device: d_guide is not 16-byte aligned (two float4s per pixel)");
	if (const char* const refused = refused_guide_flag(flags))
		return fail(RT_HIP_UNSUPPORTED, "rt_hip_guide_device: %s is not available for the guide (0x%x): it takes RT_HIP_FLAG_TRACE_BOXES, and RT_HIP_FLAG_SM_MATERIALS, RT_HIP_FLAG_BVH, RT_HIP_FLAG_BVH_DEVICE_BUILD and RT_HIP_FLAG_STATS without effect", refused, flags);
	if (!ctx->have_scene)
		return fail(RT_HIP_NO_SCENE, "rt_hip_guide_device: no scene uploaded");
	bool trace_boxes = false;
	if (const rt_hip_status st = guide_boxes("rt_hip_guide_device", ctx, flags, &trace_boxes))
		return st;
	try
	{
		RT_HIP_TRY(hipSetDevice(ctx->device)); // (a multi-GPU, rank or frame-group context: the root member, like the other device-level calls)
		return launch_guide(ctx, width, height, ctx->inverse_view_projection, trace_boxes, d_guide, static_cast<hipStream_t>(stream));
	}
	catch (const std::exception& e)
	{
		return fail(RT_HIP_RUNTIME_ERROR, "rt_hip_guide_device: %s", e.what());
	}
}

extern "C" rt_hip_status rt_hip_denoise_device(rt_hip_ctx* ctx,
											   uint32_t width,
											   uint32_t height,
											   const float* d_rgb_in,
											   const float* d_guide,
											   const rt_hip_denoise_params* params,
											   float* d_rgb_out,
											   uint32_t* d_rgba8_out,
											   void* stream)
{
	rt_hip_denoise_params p; // (what is wrong with the parameters is said before the context is looked at)
	if (const rt_hip_status st = resolve_params("rt_hip_denoise_device", params, p))
		return st;
	if (!ctx || !d_rgb_in || !d_guide || (!d_rgb_out && !d_rgba8_out))
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_denoise_device: NULL argument");
	if (!width || !height || width > max_frame_side || height > max_frame_side)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_denoise_device: frame %ux%u (1 .. %u a side)", width, height, max_frame_side);
	if (reinterpret_cast<uintptr_t>(d_guide) % 16u)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_denoise_device: d_guide is not 16-byte aligned (two float4s per pixel)");
	const size_t rgb_bytes = static_cast<size_t>(width) * height * 3u * sizeof(float);
	if (const rt_hip_status st = refuse_overlaps("rt_hip_denoise_device", { { d_rgb_out, rgb_bytes, "d_rgb_out" } }, { { d_rgb_in, rgb_bytes, "d_rgb_in" } }, "every pixel reads its neighbours' input"))
		return st;
	try
	{
		RT_HIP_TRY(hipSetDevice(ctx->device));
		return launch_filter(ctx, width, height, d_rgb_in, d_guide, p, d_rgb_out, d_rgba8_out, static_cast<hipStream_t>(stream));
	}
	catch (const std::exception& e)
	{
		return fail(RT_HIP_RUNTIME_ERROR, "rt_hip_denoise_device: %s", e.what());
	}
}

extern "C" rt_hip_status rt_hip_denoise_progressive(rt_hip_ctx* ctx, const rt_hip_denoise_params* params, uint32_t* pixels_rgba8888, float* rgb_f32, float* render_ms)
{
	rt_hip_denoise_params p; // (said before the context is looked at)
	if (const rt_hip_status st = resolve_params("rt_hip_denoise_progressive", params, p))
		return st;
	if (!ctx || !pixels_rgba8888)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_denoise_progressive: NULL argument");
	if (const rt_hip_status st = single_context_only("rt_hip_denoise_progressive", ctx))
		return st;
	const pass_state& in_flight = ctx->progressive; // (a read-only look: the accumulation is not touched)
	if (!in_flight.started || !in_flight.samples_done || !ctx->have_scene)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_denoise_progressive: no accumulation in flight (rt_hip_render_progressive has not delivered a pass on this context, or its last pass failed)");
	const uint32_t width = in_flight.key.width, height = in_flight.key.height;
	if (width > max_frame_side || height > max_frame_side)
		return fail(RT_HIP_UNSUPPORTED, "rt_hip_denoise_progressive: frame %ux%u (at most %u a side)", width, height, max_frame_side);
	const size_t pixels = static_cast<size_t>(width) * height;
	const size_t rgb_bytes = pixels * 3u * sizeof(float), rgba_bytes = pixels * sizeof(uint32_t);
	if (ctx->accum.bytes < rgb_bytes)
		return fail(RT_HIP_RUNTIME_ERROR, "rt_hip_denoise_progressive: the accumulator is smaller than its frame");
	try
	{
		RT_HIP_TRY(hipSetDevice(ctx->device));
		denoise_state& d = ctx->denoise;
		const hipStream_t s = ctx->stream;
		if (!d.begin)
			RT_HIP_TRY(hipEventCreate(&d.begin));
		if (!d.end)
			RT_HIP_TRY(hipEventCreate(&d.end));
		RT_HIP_TRY(d.mean.reserve(rgb_bytes));
		RT_HIP_TRY(d.packed.reserve(rgba_bytes));
		if (rgb_f32)
			RT_HIP_TRY(d.filtered.reserve(rgb_bytes));
		staged_results results{ d.staging, rgba_bytes, rgb_f32 ? rgb_bytes : 0u, false };
		RT_HIP_TRY(results.reserve());
		// the guide belongs to the accumulation: built when the kept one is another frame's (its key differs), kept otherwise
		const bool fresh_guide = !d.have_guide || !same_frame(d.guide_key, in_flight.key) || d.guide.bytes < pixels * denoise::guide_words * sizeof(float);
		if (fresh_guide)
		{
			if (ctx->scene_fingerprint != in_flight.key.scene_fingerprint)
				return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_denoise_progressive: the resident scene is no longer the accumulation's (another scene was uploaded since its last pass)");
			d.have_guide = false;
			RT_HIP_TRY(d.guide.reserve(pixels * denoise::guide_words * sizeof(float)));
		}
		frame_scope scope(s, true); // whatever was enqueued has finished before anything returns
		RT_HIP_TRY(hipEventRecord(d.begin, s));
		if (fresh_guide) // (the frame's flags: passes take no RT_HIP_FLAG_TRACE_BOXES, and the others do not change a first hit)
			if (const rt_hip_status st = launch_guide(ctx, width, height, in_flight.key.inverse_view_projection, false, d.guide.as<float>(), s))
				return st;
		hipLaunchKernelGGL(mean_frame, dim3(static_cast<uint32_t>((pixels * 3u + block_threads - 1u) / block_threads)), dim3(block_threads), 0, s, pixels * 3u, ctx->accum.as<float>(), static_cast<float>(in_flight.samples_done), d.mean.as<float>());
		RT_HIP_TRY(hipGetLastError());
		if (const rt_hip_status st = launch_filter(ctx, width, height, d.mean.as<float>(), d.guide.as<float>(), p, rgb_f32 ? d.filtered.as<float>() : nullptr, d.packed.as<uint32_t>(), s))
			return st;
		RT_HIP_TRY(hipEventRecord(d.end, s));
		if (const rt_hip_status st = results.deliver(scope, d.packed.ptr, d.filtered.ptr, nullptr, pixels_rgba8888, rgb_f32, nullptr))
			return st;
		if (fresh_guide)
		{
			d.guide_key = in_flight.key;
			d.have_guide = true;
		}
		if (render_ms)
			*render_ms = elapsed_or_zero(d.begin, d.end);
		return ok();
	}
	catch (const std::exception& e)
	{
		return fail(RT_HIP_RUNTIME_ERROR, "rt_hip_denoise_progressive: %s", e.what());
	}
}
