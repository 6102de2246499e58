// rt_amd/csrc/bloom.hip — bloom for HDR frames: the four kernels (bloom_prefilter, bloom_down, bloom_up,
// bloom_composite), the device-level entry point rt_hip_bloom_device, the three host-only helpers of include/rt_hip.h, and the drop-in
// rt_hip_render_bloomed — one call, one frame: trace, bloom, meter, map.
//
// A translation unit of its own: it changes nothing of the render kernels, launches the frame through what render.hip already offers
// (render_device) and maps it through what tonemap.hip offers (launch_tonemap).  What a bright pixel, a tap sum and a clamped index ARE is
// bloom_rules.hpp's, the text the CPU restatement (tests/native/bloom_reference.cpp) runs too; here is only how the texels reach the
// rules.  Every texel of every level is computed by exactly one lane, from values complete before its launch began, in the rules' order:
// nothing is accumulated across lanes, so there is nothing for an order of arrival to change.
#include "internal.hpp"
#include "bloom.hpp"
#include "bloom_rules.hpp"

namespace rt_hip
{
namespace tonemap
{
	namespace leaf // (tonemap_rules.hpp wants its leaf; of that header the drop-in reads the state record's layout alone)
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
	// ---- the one-lane-per-texel kernels: workgroups of 64 x 4 texels, a 1-D grid of them ----------------------------------------------
	// A wave is 64 consecutive texels of one row: 768 contiguous bytes per load or store instruction triple.  The grid is tiles_x x
	// tiles_y workgroups in ONE dimension (blockIdx.x = ty * tiles_x + tx: at most 512 x 8192), so no grid dimension but x depends on a
	// frame side.
	constexpr uint32_t strip_w = 64, strip_h = block_threads / strip_w;

	struct texel_at
	{
		uint32_t x, y;
		bool inside;
	};
	__device__ __forceinline__ texel_at strip_texel(uint32_t tiles_x, uint32_t w, uint32_t h)
	{
		const uint32_t tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
		const uint32_t x = tx * strip_w + (threadIdx.x & (strip_w - 1u)), y = ty * strip_h + threadIdx.x / strip_w;
		return { x, y, x < w && y < h };
	}
	__device__ __forceinline__ bloom::rgb load_rgb(const float* image, uint32_t w, uint32_t x, uint32_t y)
	{
		const size_t at = (static_cast<size_t>(y) * w + x) * 3u;
		return { image[at], image[at + 1u], image[at + 2u] };
	}
	__device__ __forceinline__ void store_rgb(float* image, uint32_t w, uint32_t x, uint32_t y, bloom::rgb v)
	{
		const size_t at = (static_cast<size_t>(y) * w + x) * 3u;
		image[at] = v.r;
		image[at + 1u] = v.g;
		image[at + 2u] = v.b;
	}
	// the tent over `coarse` (wc x hc) for the fine texel (x, y): rows first, then the two rows
	__device__ __forceinline__ bloom::rgb tent(const float* coarse, uint32_t wc, uint32_t hc, uint32_t x, uint32_t y)
	{
		const uint32_t X = x >> 1, Xn = bloom::tent_neighbour(x, wc), Y = y >> 1, Yn = bloom::tent_neighbour(y, hc);
		const bloom::rgb row = bloom::tent2(load_rgb(coarse, wc, X, Y), load_rgb(coarse, wc, Xn, Y));
		const bloom::rgb row_n = bloom::tent2(load_rgb(coarse, wc, X, Yn), load_rgb(coarse, wc, Xn, Yn));
		return bloom::tent2(row, row_n);
	}

	// ---- bloom_prefilter: one lane per level-0 texel — the bright pass of its 2 x 2 full-size pixels, averaged --------------------------
	__global__ __launch_bounds__(block_threads) void bloom_prefilter(const uint32_t W, const uint32_t H, const uint32_t w0, const uint32_t h0, const uint32_t tiles_x, const float threshold, const float knee, const float* __restrict__ in,
																	 float* __restrict__ level0)
	{
		const texel_at t = strip_texel(tiles_x, w0, h0);
		if (!t.inside)
			return;
		const uint32_t x0 = bloom::quad_index(t.x, 0u, W), x1 = bloom::quad_index(t.x, 1u, W), y0 = bloom::quad_index(t.y, 0u, H), y1 = bloom::quad_index(t.y, 1u, H);
		const auto bright_at = [&](uint32_t x, uint32_t y)
		{
			const bloom::rgb c = load_rgb(in, W, x, y);
			return bloom::bright(c.r, c.g, c.b, threshold, knee);
		};
		store_rgb(level0, w0, t.x, t.y, bloom::box4(bright_at(x0, y0), bright_at(x1, y0), bright_at(x0, y1), bright_at(x1, y1)));
	}

	// ---- bloom_down: 256 lanes = 16 x 16 texels of the next level, the 35 x 35 source texels around them staged in LDS -----------------
	// Output (X, Y) is the separable binomial around source texel (2 X, 2 Y): the tile's outputs read source columns 32 tx - 2 ..
	// 32 tx + 32 and as many rows, indices clamped to the level WHEN STAGED, so the passes below index the tile alone.
	//   1. stage    35 x 35 texels x 3 channels, lanes over the tile's floats in memory order (a tile row is 105 contiguous floats)
	//   2. rows     35 rows x 16 outputs x 3 channels of binomial5 over tile columns 2 ox .. 2 ox + 4, into `rows`
	//   3. columns  lane (ox, oy): binomial5 over rows 2 oy .. 2 oy + 4 of `rows`, x 1 / 256, one store
	// LDS: 3 x 1227 + 3 x 864 floats, 24.5 KiB a workgroup: six workgroups a compute unit.
	// Banking (ds_read_b32 / ds_write_b32: bank = dword address mod 32, conflicts within a 32-lane half):
	//   - the channels are PLANES (tile[c][row][col]), not interleaved: interleaved, pass 2's lanes would stride 6 dwords.
	//   - a tile row is 35 dwords.  In pass 2 a half is two tile rows x 16 outputs reading dwords 2 ox + k: 16 banks of one parity per
	//     row, and the odd row length puts the second row on the other parity: no conflict.
	//   - a plane is 1227 dwords, 11 mod 32: in pass 1 consecutive lanes write channels 0 1 2 of consecutive texels, banks
	//     11 c + col — a half's eleven texels land on 0 .. 10, 11 .. 21, 22 .. 31.
	//   - `rows` keeps rows in PAIRS of 48 dwords, row r at (r >> 1) * 48 + (r & 1) * 16: pass 2's half writes one even row and the
	//     next, 32 consecutive dwords; pass 3's half is outputs oy, oy + 1 reading rows 2 oy + k and 2 oy + 2 + k, one pair on, which
	//     is 48 = 16 mod 32 dwords away: the two 16-lane rows land on different halves of the banks.  No conflict in either.
	constexpr uint32_t down_out = 16, down_src = 2u * down_out + 3u; // 35
	constexpr uint32_t down_plane = 1227, down_rows_plane = ((down_src + 1u) / 2u) * 48u; // 864
	static_assert(down_plane >= down_src * down_src && down_plane % 32u == 11u && down_out * down_out == block_threads);
	__device__ __forceinline__ uint32_t rows_at(uint32_t row, uint32_t ox) { return (row >> 1) * 48u + (row & 1u) * 16u + ox; }

	__global__ __launch_bounds__(block_threads) void bloom_down(const uint32_t w, const uint32_t h, const uint32_t wn, const uint32_t hn, const uint32_t tiles_x, const float* __restrict__ src, float* __restrict__ dst)
	{
		__shared__ float tile[3u * down_plane];
		__shared__ float rows[3u * down_rows_plane];
		const uint32_t tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
		const int32_t sx0 = static_cast<int32_t>(tx * 2u * down_out) - 2, sy0 = static_cast<int32_t>(ty * 2u * down_out) - 2;
		constexpr uint32_t row_floats = down_src * 3u;
		for (uint32_t i = threadIdx.x; i < down_src * row_floats; i += block_threads)
		{
			const uint32_t row = i / row_floats, rest = i - row * row_floats, col = rest / 3u, c = rest - col * 3u;
			const uint32_t sx = bloom::clamp_index(sx0 + static_cast<int32_t>(col), w), sy = bloom::clamp_index(sy0 + static_cast<int32_t>(row), h);
			tile[c * down_plane + row * down_src + col] = src[(static_cast<size_t>(sy) * w + sx) * 3u + c];
		}
		__syncthreads();
		for (uint32_t i = threadIdx.x; i < down_src * down_out; i += block_threads)
		{
			const uint32_t row = i / down_out, ox = i % down_out;
			for (uint32_t c = 0; c < 3u; c++)
			{
				const float* const t = tile + c * down_plane + row * down_src + 2u * ox;
				rows[c * down_rows_plane + rows_at(row, ox)] = bloom::binomial5(t[0], t[1], t[2], t[3], t[4]);
			}
		}
		__syncthreads();
		const uint32_t ox = threadIdx.x % down_out, oy = threadIdx.x / down_out;
		const uint32_t X = tx * down_out + ox, Y = ty * down_out + oy;
		if (X >= wn || Y >= hn)
			return;
		float v[3];
		for (uint32_t c = 0; c < 3u; c++)
		{
			const float* const r = rows + c * down_rows_plane;
			v[c] = bloom::down_finish(bloom::binomial5(r[rows_at(2u * oy, ox)], r[rows_at(2u * oy + 1u, ox)], r[rows_at(2u * oy + 2u, ox)], r[rows_at(2u * oy + 3u, ox)], r[rows_at(2u * oy + 4u, ox)]));
		}
		store_rgb(dst, wn, X, Y, { v[0], v[1], v[2] });
	}

	// ---- bloom_up: one lane per texel of the finer level, in place: up[i] = level[i] + scatter x tent(up[i + 1]) -----------------------
	// A lane reads its own texel of `fine` and four of `coarse`, which is another level: nothing a lane reads is written in this launch.
	__global__ __launch_bounds__(block_threads) void bloom_up(const uint32_t w, const uint32_t h, const uint32_t wc, const uint32_t hc, const uint32_t tiles_x, const float scatter, const float* __restrict__ coarse, float* __restrict__ fine)
	{
		const texel_at t = strip_texel(tiles_x, w, h);
		if (!t.inside)
			return;
		store_rgb(fine, w, t.x, t.y, bloom::up_sum(load_rgb(fine, w, t.x, t.y), scatter, tent(coarse, wc, hc, t.x, t.y)));
	}

	// ---- bloom_composite: one lane per full-size pixel: layer = tent(up[0]), out = in + gain x layer -----------------------------------
	// `in` and `out` may be the same frame (not __restrict__): a lane reads its own pixel's three floats before it stores them.
	__global__ __launch_bounds__(block_threads) void bloom_composite(const uint32_t W, const uint32_t H, const uint32_t w0, const uint32_t h0, const uint32_t tiles_x, const float gain, const float* __restrict__ level0, const float* in, float* out,
																	 float* layer_out)
	{
		const texel_at t = strip_texel(tiles_x, W, H);
		if (!t.inside)
			return;
		const bloom::rgb layer = tent(level0, w0, h0, t.x, t.y);
		if (out)
			store_rgb(out, W, t.x, t.y, bloom::composite(load_rgb(in, W, t.x, t.y), gain, layer));
		if (layer_out)
			store_rgb(layer_out, W, t.x, t.y, layer);
	}

	// `params`, or the defaults; refused with the field's name
	rt_hip_status resolve_bloom(const char* who, const rt_hip_bloom_params* params, rt_hip_bloom_params& out)
	{
		out = params ? *params : default_bloom_params();
		const bloom_check checked = check_bloom_params(out);
		if (checked.status)
			return fail(checked.status, "%s: %s", who, checked.message);
		return ok();
	}

	uint32_t strips_x(uint32_t w) { return (w + strip_w - 1u) / strip_w; }
	uint32_t strips(uint32_t w, uint32_t h) { return strips_x(w) * ((h + strip_h - 1u) / strip_h); }

	// the 2 x levels launches on device buffers (everything checked by the caller; the context's device is current)
	rt_hip_status launch_bloom(rt_hip_ctx* ctx, uint32_t width, uint32_t height, const float* d_in, const rt_hip_bloom_params& p, float* d_out, float* d_layer, hipStream_t stream)
	{
		const bloom_plan plan = plan_bloom(width, height, p);
		RT_HIP_TRY(ctx->bloom.pyramid.reserve(plan.scratch_bytes));
		float* const pyramid = ctx->bloom.pyramid.as<float>();
		const auto level = [&](uint32_t i) { return pyramid + plan.level[i].offset; };
		const bloom_level* const l = plan.level;
		hipLaunchKernelGGL(bloom_prefilter, dim3(strips(l[0].width, l[0].height)), dim3(block_threads), 0, stream, width, height, l[0].width, l[0].height, strips_x(l[0].width), p.threshold, p.knee, d_in, level(0));
		RT_HIP_TRY(hipGetLastError());
		for (uint32_t i = 0; i + 1u < plan.levels; i++)
		{
			const uint32_t tiles_x = (l[i + 1u].width + down_out - 1u) / down_out, tiles_y = (l[i + 1u].height + down_out - 1u) / down_out;
			hipLaunchKernelGGL(bloom_down, dim3(tiles_x * tiles_y), dim3(block_threads), 0, stream, l[i].width, l[i].height, l[i + 1u].width, l[i + 1u].height, tiles_x, level(i), level(i + 1u));
			RT_HIP_TRY(hipGetLastError());
		}
		for (uint32_t i = plan.levels - 1u; i-- > 0u;)
		{
			hipLaunchKernelGGL(bloom_up, dim3(strips(l[i].width, l[i].height)), dim3(block_threads), 0, stream, l[i].width, l[i].height, l[i + 1u].width, l[i + 1u].height, strips_x(l[i].width), p.scatter, level(i + 1u), level(i));
			RT_HIP_TRY(hipGetLastError());
		}
		hipLaunchKernelGGL(bloom_composite, dim3(strips(width, height)), dim3(block_threads), 0, stream, width, height, l[0].width, l[0].height, strips_x(width), plan.gain, level(0), d_in, d_out, d_layer);
		RT_HIP_TRY(hipGetLastError());
		return ok();
	}
}
}

using namespace rt_hip;

extern "C" rt_hip_status rt_hip_bloom_default_params(rt_hip_bloom_params* out_params)
{
	if (!out_params)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_bloom_default_params: NULL argument");
	*out_params = default_bloom_params();
	return ok();
}

extern "C" rt_hip_status rt_hip_bloom_from_spec(const char* spec, rt_hip_bloom_params* out_params)
{
	const bloom_check checked = bloom_from_spec(spec, out_params);
	if (checked.status)
		return fail(checked.status, "%s", checked.message);
	return ok();
}

extern "C" rt_hip_status rt_hip_bloom_plan(uint32_t width, uint32_t height, const rt_hip_bloom_params* params, rt_hip_bloom_info* out_info)
{
	rt_hip_bloom_params p;
	if (const rt_hip_status st = resolve_bloom("rt_hip_bloom_plan", params, p))
		return st;
	if (!out_info)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_bloom_plan: NULL argument");
	if (!width || !height || width > max_frame_side || height > max_frame_side)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_bloom_plan: frame %ux%u (1 .. %u a side)", width, height, max_frame_side);
	const bloom_plan plan = plan_bloom(width, height, p);
	*out_info = { plan.levels, plan.level[plan.levels - 1u].width, plan.level[plan.levels - 1u].height, plan.scratch_bytes };
	return ok();
}

extern "C" rt_hip_status rt_hip_bloom_device(rt_hip_ctx* ctx, uint32_t width, uint32_t height, const float* d_rgb_in, const rt_hip_bloom_params* params, float* d_rgb_out, float* d_layer_out, void* stream)
{
	rt_hip_bloom_params p; // (what is wrong with the parameters is said before the context is looked at)
	if (const rt_hip_status st = resolve_bloom("rt_hip_bloom_device", params, p))
		return st;
	if (!ctx || !d_rgb_in)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_bloom_device: NULL argument");
	if (!d_rgb_out && !d_layer_out)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_bloom_device: NULL argument (d_rgb_out and d_layer_out are both NULL: nothing to write)");
	if (!width || !height || width > max_frame_side || height > max_frame_side)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_bloom_device: frame %ux%u (1 .. %u a side)", width, height, max_frame_side);
	if (reinterpret_cast<uintptr_t>(d_rgb_in) % 4u || reinterpret_cast<uintptr_t>(d_rgb_out) % 4u || reinterpret_cast<uintptr_t>(d_layer_out) % 4u)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_bloom_device: d_rgb_in, d_rgb_out or d_layer_out is not 4-byte aligned");
	const size_t bytes = static_cast<size_t>(width) * height * 3u * sizeof(float);
	float* const separate_out = d_rgb_out == d_rgb_in ? nullptr : d_rgb_out; // in place: exactly the input frame, pixel on pixel
	if (const rt_hip_status st = refuse_overlaps("rt_hip_bloom_device", { { separate_out, bytes, "d_rgb_out" }, { d_layer_out, bytes, "d_layer_out" } }, { { d_rgb_in, bytes, "d_rgb_in" } }, "only d_rgb_out == d_rgb_in exactly is in place"))
		return st;
	try
	{
		RT_HIP_TRY(hipSetDevice(ctx->device)); // (a multi-GPU, rank or frame-group context: the root member, like the other device-level calls)
		return launch_bloom(ctx, width, height, d_rgb_in, p, d_rgb_out, d_layer_out, static_cast<hipStream_t>(stream));
	}
	catch (const std::exception& e)
	{
		return fail(RT_HIP_RUNTIME_ERROR, "rt_hip_bloom_device: %s", e.what());
	}
}

extern "C" rt_hip_status rt_hip_render_bloomed(rt_hip_ctx* ctx,
											   const rt_hip_scene* scene,
											   uint32_t* pixels_rgba8888,
											   uint32_t width,
											   uint32_t height,
											   uint64_t seed,
											   uint32_t flags,
											   const rt_hip_bloom_params* bloom_params,
											   const rt_hip_tonemap_params* tonemap_params,
											   float* rgb_f32,
											   rt_hip_stats* stats,
											   rt_hip_tonemap_info* out_tonemap_info)
{
	rt_hip_bloom_params b; // (said before the context is looked at)
	if (const rt_hip_status st = resolve_bloom("rt_hip_render_bloomed", bloom_params, b))
		return st;
	rt_hip_tonemap_params p;
	if (const rt_hip_status st = resolve_tonemap("rt_hip_render_bloomed", tonemap_params, p))
		return st;
	if (!ctx || !scene || !pixels_rgba8888)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_render_bloomed: NULL argument");
	if (!width || !height || width > max_frame_side || height > max_frame_side)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_render_bloomed: frame %ux%u (1 .. %u a side)", width, height, max_frame_side);
	if (flags & RT_HIP_FLAG_PREVIEW) // (the flags are refused before the context is looked at)
		return fail(RT_HIP_UNSUPPORTED, "rt_hip_render_bloomed: RT_HIP_FLAG_PREVIEW is not available for bloomed frames (0x%x): the preview has no float mean", flags);
	if (flags & RT_HIP_FLAG_PERSISTENT_FRAME)
		return fail(RT_HIP_UNSUPPORTED, "rt_hip_render_bloomed: RT_HIP_FLAG_PERSISTENT_FRAME is not available for bloomed frames (0x%x): the pixels come from a device buffer", flags);
	if (flags & ~(render_flag_mask | static_cast<uint32_t>(RT_HIP_FLAG_STATS)))
		return fail(RT_HIP_UNSUPPORTED, "rt_hip_render_bloomed: unknown flag bits 0x%x", flags);
	if (const rt_hip_status st = single_context_only("rt_hip_render_bloomed", ctx))
		return st;
	const size_t pixels = static_cast<size_t>(width) * height;
	const size_t rgb_bytes = pixels * 3u * sizeof(float), rgba_bytes = pixels * sizeof(uint32_t);
	const bool keep_stats = stats || (flags & RT_HIP_FLAG_STATS);
	try
	{
		RT_HIP_TRY(hipSetDevice(ctx->device));
		scene_request request;
		if (const rt_hip_status st = resident_scene(ctx, scene, request))
			return st;

		bloom_state& t = ctx->bloom;
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
		// 1. the one-shot frame, by the launch rt_hip_render_device makes (its packed pixels are overwritten by 3.)
		if (const rt_hip_status st = render_device(ctx, width, height, seed, flags & render_flag_mask, nullptr, t.packed.as<uint32_t>(), t.traced.as<float>(), s, false, keep_stats, false, nullptr, true))
			return st;
		// 2. the pyramid and the composite, in place
		if (const rt_hip_status st = launch_bloom(ctx, width, height, t.traced.as<float>(), b, t.traced.as<float>(), nullptr, s))
			return st;
		// 3. the histogram, the exposure, the pixels, in place
		if (const rt_hip_status st = launch_tonemap(ctx, width, height, t.traced.as<float>(), p, t.record.as<uint32_t>(), rgb_f32 ? t.traced.as<float>() : nullptr, t.packed.as<uint32_t>(), s))
			return st;
		if (keep_stats)
			RT_HIP_TRY(hipEventRecord(t.end, s));
		uint32_t record[tonemap::state_words] = {};
		if (const rt_hip_status st = results.deliver(scope, t.packed.ptr, t.traced.ptr, t.record.ptr, pixels_rgba8888, rgb_f32, record))
			return st;
		t.width = width, t.height = height;
		if (out_tonemap_info)
			*out_tonemap_info = { tonemap::float_of(record[0]), tonemap::float_of(record[1]), record[2], record[3], record[4], record[5] };
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
		return fail(RT_HIP_RUNTIME_ERROR, "rt_hip_render_bloomed: %s", e.what());
	}
}
