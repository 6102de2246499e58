// rt_amd/csrc/tonemap.hip — tone mapping for HDR frames: the three kernels (luminance_histogram,
// exposure_from_histogram, tonemap_frame), the device-level entry point rt_hip_tonemap_device, the two host-only helpers of
// include/rt_hip.h, and the drop-in rt_hip_render_tonemapped — one call, one frame: trace, meter, map.
//
// A translation unit of its own: it changes nothing of the render kernels and launches the frame through what render.hip already
// offers (render_device).  What a pixel's luminance, its bin, the exposure and the mapped pixel ARE is tonemap_rules.hpp's, the text
// the CPU restatement (tests/native/tonemap_reference.cpp) runs too; here is only how the pixels reach the rules and how the
// histogram is gathered.  The exposure goes from the histogram to the pixels through the state record in device memory: the host
// never sees it on the way.
#include "internal.hpp"
#include "tonemap.hpp"

namespace rt_hip
{
namespace tonemap
{
	namespace leaf // the contract's own finish, handed to the rules (tonemap_rules.hpp has the list)
	{
		__device__ __forceinline__ uint32_t pack_mean(float r, float g, float b) { return rt_hip::pack_mean({ r, g, b }); }
	}
}
}
#include "tonemap_rules.hpp"

#include <exception>

namespace rt_hip
{
namespace
{
	constexpr uint32_t waves = block_threads / 64u;
	constexpr uint32_t grid_per_compute_unit = 2; // luminance_histogram's grid is at most this many workgroups per compute unit

	// ---- luminance_histogram: 256 bins of the frame's log2 luminance, and the pixels that are not metered ---------------------------
	// A lane takes RUNS of 4 consecutive pixels — 12 floats, three 16-byte loads, aligned whenever the frame is — and the workgroups
	// stride over the runs; the W x H mod 4 pixels behind the last run are the first workgroup's, one lane each.  Every wave counts
	// into a 256-bin histogram of its own in LDS (integer atomics: 4 KiB a workgroup); behind one barrier lane b sums bin b of the
	// four and adds it to the frame's with ONE global integer atomic, if it is not empty.  All integers: no order can matter.
	__device__ __forceinline__ void count_pixel(uint32_t* wave_bins, uint32_t& skipped, float r, float g, float b)
	{
		const float y = tonemap::luminance(r, g, b);
		if (tonemap::counted(y))
			atomicAdd(wave_bins + tonemap::bin_of(y), 1u);
		else
			skipped++;
	}

	__global__ __launch_bounds__(block_threads) void luminance_histogram(const uint32_t pixels, const float* rgb, uint32_t* __restrict__ histogram)
	{
		__shared__ uint32_t bins[waves][tonemap::bins];
		__shared__ uint32_t skipped_here;
		for (uint32_t w = 0; w < waves; w++)
			bins[w][threadIdx.x] = 0u;
		if (threadIdx.x == 0u)
			skipped_here = 0u;
		__syncthreads();

		uint32_t* const mine = bins[threadIdx.x / 64u];
		uint32_t skipped = 0;
		const uint32_t runs = pixels / 4u;
		const float4* const quads = reinterpret_cast<const float4*>(rgb);
		for (uint32_t run = blockIdx.x * block_threads + threadIdx.x; run < runs; run += gridDim.x * block_threads)
		{
			const size_t at = static_cast<size_t>(run) * 3u; // (run < runs: the three quads end at or before float 3 * pixels)
			const float4 a = quads[at], b = quads[at + 1u], c = quads[at + 2u];
			count_pixel(mine, skipped, a.x, a.y, a.z);
			count_pixel(mine, skipped, a.w, b.x, b.y);
			count_pixel(mine, skipped, b.z, b.w, c.x);
			count_pixel(mine, skipped, c.y, c.z, c.w);
		}
		if (blockIdx.x == 0u && threadIdx.x < (pixels & 3u)) // the tail: pixels 4 * runs .. pixels - 1
		{
			const size_t at = (static_cast<size_t>(runs) * 4u + threadIdx.x) * 3u;
			count_pixel(mine, skipped, rgb[at], rgb[at + 1u], rgb[at + 2u]);
		}
		if (skipped)
			atomicAdd(&skipped_here, skipped);
		__syncthreads();

		uint32_t sum = 0;
		for (uint32_t w = 0; w < waves; w++)
			sum += bins[w][threadIdx.x];
		if (sum)
			atomicAdd(histogram + threadIdx.x, sum);
		if (threadIdx.x == 0u && skipped_here)
			atomicAdd(histogram + tonemap::bins, skipped_here);
	}
	static_assert(block_threads == tonemap::bins, "lane b of a workgroup owns bin b");

	// ---- exposure_from_histogram: one workgroup, one lane, a serial walk over 256 bins (tonemap::meter) ------------------------------
	// Two passes over 1 KiB and one 64-bit division, once per frame: there is nothing here for a scan to win.
	__global__ __launch_bounds__(64) void exposure_from_histogram(const rt_hip_tonemap_params params, const uint32_t* __restrict__ histogram, uint32_t* __restrict__ state)
	{
		if (threadIdx.x != 0u || blockIdx.x != 0u)
			return;
		const tonemap::metered m = tonemap::meter(histogram, params);
		const float exposure = tonemap::adapt(state[0], m.target, params.adaptation);
		state[0] = tonemap::bits_of(exposure);
		state[1] = tonemap::bits_of(m.target);
		state[2] = m.counted;
		state[3] = histogram[tonemap::bins];
		state[4] = m.kept;
		state[5] = m.mean_q8;
		state[6] = 0u;
		state[7] = 0u;
	}

	// ---- tonemap_frame: one lane per pixel ------------------------------------------------------------------------------------------
	// `in` and `out` may be the same frame (not __restrict__): a lane reads its own pixel's three floats before it stores them.
	__global__ __launch_bounds__(block_threads) void tonemap_frame(const uint32_t pixels, const uint32_t curve, const float white2, const uint32_t* state, const float* in, float* out, uint32_t* rgba)
	{
		const float exposure = tonemap::float_of(state[0]); // (one uniform load)
		const uint32_t pixel = blockIdx.x * block_threads + threadIdx.x;
		if (pixel >= pixels)
			return;
		const size_t at = static_cast<size_t>(pixel) * 3u;
		const tonemap::rgb o = tonemap::map_pixel(in[at], in[at + 1u], in[at + 2u], exposure, curve, white2);
		if (out)
		{
			out[at] = o.r;
			out[at + 1u] = o.g;
			out[at + 2u] = o.b;
		}
		if (rgba)
			rgba[pixel] = tonemap::finish(o);
	}

}

	// (the two below are bloom.hip's too: declared in internal.hpp)
	// `params`, or the defaults; refused with the field's name
	rt_hip_status resolve_tonemap(const char* who, const rt_hip_tonemap_params* params, rt_hip_tonemap_params& out)
	{
		out = params ? *params : default_tonemap_params();
		const tonemap_check checked = check_tonemap_params(out);
		if (checked.status)
			return fail(checked.status, "%s: %s", who, checked.message);
		return ok();
	}

	// the three launches on device buffers (everything checked by the caller; the context's device is current)
	rt_hip_status launch_tonemap(rt_hip_ctx* ctx, uint32_t width, uint32_t height, const float* d_in, const rt_hip_tonemap_params& p, uint32_t* d_state, float* d_out, uint32_t* d_rgba, hipStream_t stream)
	{
		const uint32_t pixels = width * height; // (at most 2^30: max_frame_side)
		if (p.exposure > 0.0f)
		{
			// manual: exposure and target are the parameter's bits, the words that describe a histogram are 0 — two fills, no kernel
			RT_HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_state), static_cast<int>(tonemap::bits_of(p.exposure)), 2u, stream));
			RT_HIP_TRY(hipMemsetAsync(d_state + 2, 0, (tonemap::state_words - 2u) * sizeof(uint32_t), stream));
		}
		else
		{
			RT_HIP_TRY(ctx->tonemap.histogram.reserve(tonemap::histogram_words * sizeof(uint32_t)));
			uint32_t* const histogram = ctx->tonemap.histogram.as<uint32_t>();
			RT_HIP_TRY(hipMemsetAsync(histogram, 0, tonemap::histogram_words * sizeof(uint32_t), stream));
			const uint32_t wanted = (pixels / 4u + block_threads - 1u) / block_threads, most = grid_per_compute_unit * ctx->compute_units;
			const uint32_t grid = wanted < 1u ? 1u : (wanted < most ? wanted : most);
			hipLaunchKernelGGL(luminance_histogram, dim3(grid), dim3(block_threads), 0, stream, pixels, d_in, histogram);
			RT_HIP_TRY(hipGetLastError());
			hipLaunchKernelGGL(exposure_from_histogram, dim3(1), dim3(64), 0, stream, p, histogram, d_state);
			RT_HIP_TRY(hipGetLastError());
		}
		hipLaunchKernelGGL(tonemap_frame, dim3((pixels + block_threads - 1u) / block_threads), dim3(block_threads), 0, stream, pixels, p.curve, p.white * p.white, d_state, d_in, d_out, d_rgba);
		RT_HIP_TRY(hipGetLastError());
		return ok();
	}
}

using namespace rt_hip;

extern "C" rt_hip_status rt_hip_tonemap_default_params(rt_hip_tonemap_params* out_params)
{
	if (!out_params)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_tonemap_default_params: NULL argument");
	*out_params = default_tonemap_params();
	return ok();
}

extern "C" rt_hip_status rt_hip_tonemap_from_spec(const char* spec, rt_hip_tonemap_params* out_params)
{
	const tonemap_check checked = tonemap_from_spec(spec, out_params);
	if (checked.status)
		return fail(checked.status, "%s", checked.message);
	return ok();
}

extern "C" rt_hip_status rt_hip_tonemap_device(rt_hip_ctx* ctx, uint32_t width, uint32_t height, const float* d_rgb_in, const rt_hip_tonemap_params* params, uint32_t* d_state, float* d_rgb_out, uint32_t* d_rgba8_out, void* stream)
{
	rt_hip_tonemap_params p; // (what is wrong with the parameters is said before the context is looked at)
	if (const rt_hip_status st = resolve_tonemap("rt_hip_tonemap_device", params, p))
		return st;
	if (!ctx || !d_rgb_in || !d_state)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_tonemap_device: NULL argument");
	if (!d_rgb_out && !d_rgba8_out)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_tonemap_device: NULL argument (d_rgb_out and d_rgba8_out are both NULL: nothing to write)");
	if (!width || !height || width > max_frame_side || height > max_frame_side)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_tonemap_device: frame %ux%u (1 .. %u a side)", width, height, max_frame_side);
	if (reinterpret_cast<uintptr_t>(d_rgb_in) % 16u)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_tonemap_device: d_rgb_in is not 16-byte aligned (the meter reads four pixels as three 16-byte loads)");
	if (reinterpret_cast<uintptr_t>(d_state) % 4u || reinterpret_cast<uintptr_t>(d_rgb_out) % 4u || reinterpret_cast<uintptr_t>(d_rgba8_out) % 4u)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_tonemap_device: d_state, d_rgb_out or d_rgba8_out is not 4-byte aligned");
	const size_t pixels = static_cast<size_t>(width) * height;
	float* const separate_out = d_rgb_out == d_rgb_in ? nullptr : d_rgb_out; // in place: exactly the input frame, pixel on pixel
	if (const rt_hip_status st = refuse_overlaps("rt_hip_tonemap_device", { { separate_out, pixels * 3u * sizeof(float), "d_rgb_out" }, { d_rgba8_out, pixels * sizeof(uint32_t), "d_rgba8_out" }, { d_state, tonemap::state_words * sizeof(uint32_t), "d_state" } },
												 { { d_rgb_in, pixels * 3u * sizeof(float), "d_rgb_in" } }, "only d_rgb_out == d_rgb_in exactly is in place"))
		return st;
	try
	{
		RT_HIP_TRY(hipSetDevice(ctx->device)); // (a multi-GPU, rank or frame-group context: the root member, like the other device-level calls)
		return launch_tonemap(ctx, width, height, d_rgb_in, p, d_state, d_rgb_out, d_rgba8_out, static_cast<hipStream_t>(stream));
	}
	catch (const std::exception& e)
	{
		return fail(RT_HIP_RUNTIME_ERROR, "rt_hip_tonemap_device: %s", e.what());
	}
}

extern "C" rt_hip_status rt_hip_render_tonemapped(rt_hip_ctx* ctx,
												  const rt_hip_scene* scene,
												  uint32_t* pixels_rgba8888,
												  uint32_t width,
												  uint32_t height,
												  uint64_t seed,
												  uint32_t flags,
												  const rt_hip_tonemap_params* params,
												  float* rgb_f32,
												  rt_hip_stats* stats,
												  rt_hip_tonemap_info* out_info)
{
	rt_hip_tonemap_params p; // (said before the context is looked at)
	if (const rt_hip_status st = resolve_tonemap("rt_hip_render_tonemapped", params, p))
		return st;
	if (!ctx || !scene || !pixels_rgba8888)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_render_tonemapped: NULL argument");
	if (!width || !height || width > max_frame_side || height > max_frame_side)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_render_tonemapped: frame %ux%u (1 .. %u a side)", width, height, max_frame_side);
	if (const rt_hip_status st = single_context_only("rt_hip_render_tonemapped", ctx))
		return st;
	if (flags & RT_HIP_FLAG_PREVIEW)
		return fail(RT_HIP_UNSUPPORTED, "rt_hip_render_tonemapped: RT_HIP_FLAG_PREVIEW is not available for tone-mapped frames (0x%x): the preview has no float mean", flags);
	if (flags & RT_HIP_FLAG_PERSISTENT_FRAME)
		return fail(RT_HIP_UNSUPPORTED, "rt_hip_render_tonemapped: RT_HIP_FLAG_PERSISTENT_FRAME is not available for tone-mapped frames (0x%x): the pixels come from a device buffer", flags);
	if (flags & ~(render_flag_mask | static_cast<uint32_t>(RT_HIP_FLAG_STATS)))
		return fail(RT_HIP_UNSUPPORTED, "rt_hip_render_tonemapped: unknown flag bits 0x%x", flags);
	const size_t pixels = static_cast<size_t>(width) * height;
	const size_t rgb_bytes = pixels * 3u * sizeof(float), rgba_bytes = pixels * sizeof(uint32_t);
	const bool keep_stats = stats || (flags & RT_HIP_FLAG_STATS);
	try
	{
		RT_HIP_TRY(hipSetDevice(ctx->device));
		scene_request request;
		if (const rt_hip_status st = resident_scene(ctx, scene, request))
			return st;

		tonemap_state& t = ctx->tonemap;
		const hipStream_t s = ctx->stream;
		if (!t.end)
			RT_HIP_TRY(hipEventCreate(&t.end));
		RT_HIP_TRY(t.traced.reserve(rgb_bytes));
		RT_HIP_TRY(t.packed.reserve(rgba_bytes));
		RT_HIP_TRY(t.record.reserve(tonemap::state_words * sizeof(uint32_t)));
		staged_results results{ t.staging, rgba_bytes, rgb_f32 ? rgb_bytes : 0u, true };
		results.words = tonemap::state_words;
		RT_HIP_TRY(results.reserve());

		frame_scope scope(s, true); // whatever was enqueued has finished before anything returns
		if (t.width != width || t.height != height) // another frame: the kept exposure starts over
		{
			t.width = t.height = 0;
			RT_HIP_TRY(hipMemsetAsync(t.record.ptr, 0, tonemap::state_words * sizeof(uint32_t), s));
		}
		// 1. the one-shot frame, by the launch rt_hip_render_device makes (its packed pixels are overwritten by 4.)
		if (const rt_hip_status st = render_device(ctx, width, height, seed, flags & render_flag_mask, nullptr, t.packed.as<uint32_t>(), t.traced.as<float>(), s, false, keep_stats, false, nullptr, true))
			return st;
		// 2. the histogram  3. the exposure  4. the pixels, in place
		if (const rt_hip_status st = launch_tonemap(ctx, width, height, t.traced.as<float>(), p, t.record.as<uint32_t>(), rgb_f32 ? t.traced.as<float>() : nullptr, t.packed.as<uint32_t>(), s))
			return st;
		if (keep_stats)
			RT_HIP_TRY(hipEventRecord(t.end, s));
		uint32_t record[tonemap::state_words] = {};
		if (const rt_hip_status st = results.deliver(scope, t.packed.ptr, t.traced.ptr, t.record.ptr, pixels_rgba8888, rgb_f32, record))
			return st;
		t.width = width, t.height = height;
		if (out_info)
			*out_info = { tonemap::float_of(record[0]), tonemap::float_of(record[1]), record[2], record[3], record[4], record[5] };
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
		return fail(RT_HIP_RUNTIME_ERROR, "rt_hip_render_tonemapped: %s", e.what());
	}
}
