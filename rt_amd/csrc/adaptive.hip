// rt_amd/csrc/adaptive.hip — adaptive sampling: the kernel that judges the pixels after a pass and finishes the frame
// (adaptive_update), its device-level entry point rt_hip_adaptive_update_device, one adaptive pass on the resident scene
// (rt_hip_adaptive_pass_device: the render kernels' adaptive build, then the update) and the drop-in rt_hip_render_adaptive — one call,
// one pass, delivered as rt_hip_render_progressive delivers.
//
// A translation unit of its own.  What a pixel of the update is — its moments, its verdict, the 3 x 3 stop decision — is
// adaptive_rules.hpp's, the text the CPU restatement (tests/native/adaptive_reference.cpp) runs too; a pixel is finished by
// contract.hpp's pixel_mean and pack_mean, as the render kernels finish theirs; the sequencing and the parameter check are adaptive.cpp's
// (host compiler).  Here is only how the pixel's inputs reach the rules.
#include "internal.hpp"
#include "adaptive.hpp"
#include "adaptive_rules.hpp"

#include <algorithm>
#include <exception>

namespace rt_hip
{
namespace
{
	// ---- adaptive_update: one lane per pixel, 16 x 16 pixels per workgroup -------------------------------------------------------
	// Every lane applies the update to its own pixel; the first 68 lanes also evaluate `converged` for one pixel of the tile's halo,
	// from that pixel's own buffers (nothing is stored for it: the workgroup that owns it computes the same).  The verdicts meet in an
	// 18 x 18 LDS tile; behind the barrier each lane takes the 3 x 3 AND, writes moments and state of a pixel that was active, and
	// finishes its pixel — stopped or not — from the running sum and its own sample count.  The pixels still active are counted per
	// wave with a popcount of the ballot, per workgroup in LDS, and one lane per workgroup adds the count to a word in HBM.
	// The halo lanes read words that ANOTHER workgroup owns, so nothing is updated in place: the kernel reads moments and state as the
	// pass found them and writes the new ones to a scratch image of the context, which launch_update copies back on the same stream
	// (12 bytes per pixel, device to device).
	constexpr uint32_t tile = 16, halo = tile + 2u;
	static_assert(tile * tile == block_threads, "one lane per pixel of the tile");
	constexpr uint32_t halo_pixels = 4u * tile + 4u; // 68

	__device__ __forceinline__ adaptive::update judge(size_t pixel, uint32_t pass_samples, bool first_pass, bool whole_pass, const rt_hip_adaptive_params& k, const float* __restrict__ pass_sum, const float* moments, const uint32_t* state,
													  uint32_t& state_word)
	{
		state_word = first_pass ? 0u : state[pixel];
		adaptive::pass_sum sum = { 0.0f, 0.0f, 0.0f };
		adaptive::moments before = { 0.0f, 0.0f };
		if (first_pass || !adaptive::is_stopped(state_word)) // (a stopped pixel was not traced: its pass sum is stale scratch)
		{
			if (whole_pass)
				sum = { pass_sum[pixel * 3u], pass_sum[pixel * 3u + 1u], pass_sum[pixel * 3u + 2u] };
			if (!first_pass)
				before = { moments[pixel * 2u], moments[pixel * 2u + 1u] };
		}
		return adaptive::update_pixel(sum, before, state_word, pass_samples, first_pass, whole_pass, k);
	}

	__global__ __launch_bounds__(block_threads) void adaptive_update(const uint32_t width, const uint32_t height, const uint32_t pass_samples, const uint32_t first_pass, const uint32_t whole_pass, const rt_hip_adaptive_params k,
																	   const float* __restrict__ accum, const float* __restrict__ pass_sum, const float* __restrict__ moments, const uint32_t* __restrict__ state, float* __restrict__ moments_out, uint32_t* __restrict__ state_out, uint32_t* __restrict__ out_rgba, float* __restrict__ out_rgb,
																	   uint32_t* __restrict__ active, uint32_t* __restrict__ traced)
	{
		__shared__ uint32_t verdicts[halo][halo]; // 1: converged, or outside the frame
		__shared__ uint32_t wave_active[block_threads / 64u], wave_traced[block_threads / 64u];
		const int32_t x0 = static_cast<int32_t>(blockIdx.x * tile), y0 = static_cast<int32_t>(blockIdx.y * tile);
		const uint32_t tx = threadIdx.x & (tile - 1u), ty = threadIdx.x / tile;
		const uint32_t x = blockIdx.x * tile + tx, y = blockIdx.y * tile + ty;
		const bool alive = x < width && y < height;
		const size_t pixel = static_cast<size_t>(y) * width + x;
		adaptive::update mine{};
		uint32_t state_word = 0u;
		if (alive)
			mine = judge(pixel, pass_samples, first_pass != 0u, whole_pass != 0u, k, pass_sum, moments, state, state_word);
		verdicts[ty + 1u][tx + 1u] = (!alive || mine.converged) ? 1u : 0u;
		if (threadIdx.x < halo_pixels)
		{
			// the ring around the tile: the two rows of 18, then the two columns of 16
			const uint32_t h = threadIdx.x;
			uint32_t hx, hy;
			if (h < 2u * halo)
				hx = h % halo, hy = h < halo ? 0u : halo - 1u;
			else
				hx = (h - 2u * halo) < tile ? 0u : halo - 1u, hy = 1u + (h - 2u * halo) % tile;
			const int32_t qx = x0 + static_cast<int32_t>(hx) - 1, qy = y0 + static_cast<int32_t>(hy) - 1;
			uint32_t verdict = 1u;
			if (qx >= 0 && qy >= 0 && qx < static_cast<int32_t>(width) && qy < static_cast<int32_t>(height))
			{
				uint32_t unused;
				verdict = judge(static_cast<size_t>(qy) * width + static_cast<size_t>(qx), pass_samples, first_pass != 0u, whole_pass != 0u, k, pass_sum, moments, state, unused).converged ? 1u : 0u;
			}
			verdicts[hy][hx] = verdict;
		}
		__syncthreads();
		bool still_active = false;
		if (alive)
		{
			const bool stop = adaptive::stops(static_cast<int32_t>(x), static_cast<int32_t>(y), static_cast<int32_t>(width), static_cast<int32_t>(height),
											  [&](int32_t qx, int32_t qy) -> bool { return verdicts[qy - y0 + 1][qx - x0 + 1] != 0u; });
			const uint32_t after = adaptive::next_state(state_word, first_pass != 0u, mine, stop);
			// (a stopped pixel's words pass through as they are; a short pass leaves the moments alone: they are not copied back)
			if (whole_pass)
			{
				const bool kept = !first_pass && adaptive::is_stopped(state_word);
				moments_out[pixel * 2u] = kept ? moments[pixel * 2u] : mine.m.s1;
				moments_out[pixel * 2u + 1u] = kept ? moments[pixel * 2u + 1u] : mine.m.s2;
			}
			state_out[pixel] = after;
			still_active = !adaptive::is_stopped(after);
			// every pixel of every delivered frame: the running sum over the pixel's OWN sample count
			const vec3 mean = pixel_mean({ accum[pixel * 3u], accum[pixel * 3u + 1u], accum[pixel * 3u + 2u] }, static_cast<float>(adaptive::samples_of(after)));
			if (out_rgb)
				out_rgb[pixel * 3u] = mean.x, out_rgb[pixel * 3u + 1u] = mean.y, out_rgb[pixel * 3u + 2u] = mean.z;
			// (the render kernels' system-scope store: the frame may be the module's page-locked one, whose carrier copies what it finds)
			__hip_atomic_store(&out_rgba[pixel], pack_mean(mean), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
		}
		// The pixels still active: a popcount of the ballot per wave, the four waves' counts added up in LDS, ONE atomic per workgroup.
		// (One per wave, as reproject_frame counts, was measured first: 32 400 atomics on one address at 1920 x 1080 serialise at about
		// 12 ns each and made this kernel take 380 us with every pixel active against 187 us with most of them stopped —
		// profiles/r16/kernel_stats_first.txt.)
		// `traced` (nullable), counted the same way: the pixels that were active IN this pass — what the render kernel in front of this
		// one traced (state_word is 0 in the first pass), for the stats of rt_hip_adaptive_pass_device.
		const unsigned long long going_on = __ballot(still_active); // (every lane of the wave is here)
		const unsigned long long were_active = __ballot(alive && !adaptive::is_stopped(state_word));
		if ((threadIdx.x & 63u) == 0u)
		{
			wave_active[threadIdx.x >> 6] = static_cast<uint32_t>(__popcll(going_on));
			wave_traced[threadIdx.x >> 6] = static_cast<uint32_t>(__popcll(were_active));
		}
		__syncthreads();
		if ((active || traced) && threadIdx.x == 0u)
		{
			uint32_t total = 0, total_traced = 0;
			for (uint32_t w = 0; w < block_threads / 64u; w++)
				total += wave_active[w], total_traced += wave_traced[w];
			if (active && total)
				atomicAdd(active, total);
			if (traced && total_traced)
				atomicAdd(traced, total_traced);
		}
	}

	// one update step on device buffers (everything checked by the caller; ctx->device is current)
	rt_hip_status launch_update(rt_hip_ctx* ctx, uint32_t width, uint32_t height, uint32_t pass_samples, bool first_pass, bool whole_pass, const rt_hip_adaptive_params& params, const float* d_accum, const float* d_pass_sum, float* d_moments, uint32_t* d_state,
								uint32_t* d_rgba8, float* d_rgb, uint32_t* d_active, hipStream_t stream, bool count_traced = false)
	{
		if (d_active)
			RT_HIP_TRY(hipMemsetAsync(d_active, 0, sizeof(uint32_t), stream));
		const size_t pixels = static_cast<size_t>(width) * height;
		RT_HIP_TRY(ctx->adaptive.scratch.reserve((pixels * 3u + 1u) * sizeof(uint32_t))); // (the last word: the pixels traced, where they are counted)
		uint32_t* const state_out = ctx->adaptive.scratch.as<uint32_t>();
		float* const moments_out = ctx->adaptive.scratch.as<float>() + pixels;
		uint32_t* const d_traced = count_traced ? state_out + pixels * 3u : nullptr;
		if (d_traced)
			RT_HIP_TRY(hipMemsetAsync(d_traced, 0, sizeof(uint32_t), stream));
		const dim3 grid((width + tile - 1u) / tile, (height + tile - 1u) / tile);
		hipLaunchKernelGGL(adaptive_update, grid, dim3(block_threads), 0, stream, width, height, pass_samples, first_pass ? 1u : 0u, whole_pass ? 1u : 0u, params, d_accum, d_pass_sum, d_moments, d_state, moments_out, state_out, d_rgba8, d_rgb,
						   d_active, d_traced);
		RT_HIP_TRY(hipGetLastError());
		RT_HIP_TRY(hipMemcpyAsync(d_state, state_out, pixels * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream));
		if (whole_pass)
			RT_HIP_TRY(hipMemcpyAsync(d_moments, moments_out, pixels * 2u * sizeof(float), hipMemcpyDeviceToDevice, stream));
		if (d_traced)
		{
			// the count follows the pass's counters to the host on the same stream; fetch_member_stats (render.hip) waits for both
			RT_HIP_TRY(ctx->adaptive.traced.reserve(sizeof(uint32_t)));
			RT_HIP_TRY(hipMemcpyAsync(ctx->adaptive.traced.ptr, d_traced, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
			RT_HIP_TRY(hipEventRecord(ctx->counters_copied, stream));
			ctx->adaptive.traced_pass_samples = pass_samples;
		}
		return ok();
	}

	// `params`, or the defaults; refused with the field's name.  pass_size: what min_samples is held against (0: nothing)
	rt_hip_status resolve_adaptive(const char* who, const rt_hip_adaptive_params* params, uint64_t pass_size, rt_hip_adaptive_params& out)
	{
		out = params ? *params : default_adaptive_params();
		const adaptive_check checked = check_adaptive_params(out, pass_size);
		if (checked.status)
			return fail(checked.status, "%s: %s", who, checked.message);
		return ok();
	}

	// the block of rt_hip_adaptive_pass_device: accum, state, pass_sum, moments
	struct block_view
	{
		float* accum;
		uint32_t* state;
		float* pass_sum;
		float* moments;
	};
	constexpr size_t block_words = 9;
	block_view view_of(float* d_block, size_t pixels) { return { d_block, reinterpret_cast<uint32_t*>(d_block + 3u * pixels), d_block + 4u * pixels, d_block + 7u * pixels }; }

	// render + update (everything checked by the caller)
	rt_hip_status adaptive_pass(rt_hip_ctx* ctx, uint32_t width, uint32_t height, uint64_t seed, uint32_t flags, uint32_t first_sample, uint32_t n_samples, bool whole_pass, const rt_hip_adaptive_params& params, float* d_block,
								uint32_t* d_rgba8, float* d_rgb_f32, uint32_t* d_active, hipStream_t stream, bool keep_stats, bool count_traced = false)
	{
		render_pass pass = { first_sample, n_samples, d_block };
		pass.adaptive = true;
		// (the adaptive builds store no pixel: the frame is the update kernel's, and the tiles are cut as for a frame in HBM)
		if (const rt_hip_status st = render_device(ctx, width, height, seed, flags & pass_flag_mask, nullptr, d_rgba8, nullptr, stream, false, keep_stats, false, &pass))
			return st;
		const block_view b = view_of(d_block, static_cast<size_t>(width) * height);
		return launch_update(ctx, width, height, n_samples, first_sample == 0u, whole_pass, params, b.accum, b.pass_sum, b.moments, b.state, d_rgba8, d_rgb_f32, d_active, stream, count_traced && keep_stats);
	}
}
}

using namespace rt_hip;

namespace
{
	// where the most recent successful rt_hip_render_adaptive call of this process left its accumulation (rt_hip_adaptive_last_info)
	std::mutex last_info_lock;
	rt_hip_adaptive_info last_info{};
	bool have_last_info = false;
	void remember(const rt_hip_adaptive_info& info)
	{
		const std::lock_guard<std::mutex> guard(last_info_lock);
		last_info = info;
		have_last_info = true;
	}
}

extern "C" rt_hip_status rt_hip_adaptive_last_info(rt_hip_adaptive_info* out_info)
{
	if (!out_info)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_adaptive_last_info: NULL argument");
	const std::lock_guard<std::mutex> guard(last_info_lock);
	if (!have_last_info)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_adaptive_last_info: no adaptive pass has been delivered in this process");
	*out_info = last_info;
	return ok();
}

extern "C" rt_hip_status rt_hip_adaptive_default_params(rt_hip_adaptive_params* out_params)
{
	if (!out_params)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_adaptive_default_params: NULL argument");
	*out_params = default_adaptive_params();
	return ok();
}

extern "C" rt_hip_status rt_hip_adaptive_update_device(rt_hip_ctx* ctx,
														   uint32_t width,
														   uint32_t height,
														   uint32_t pass_samples,
														   uint32_t first_pass,
														   uint32_t whole_pass,
														   const rt_hip_adaptive_params* params,
														   const float* d_accum,
														   const float* d_pass_sum,
														   float* d_moments,
														   uint32_t* d_state,
														   uint32_t* d_rgba8_out,
														   float* d_rgb_out,
														   uint32_t* d_active_pixels,
														   void* stream)
{
	if (!pass_samples || pass_samples > pass_max_samples_per_pixel || (whole_pass && pass_samples % sample_chunk))
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_adaptive_update_device: pass_samples = %u (a whole pass is a multiple of %u, a short last pass anything; 1 .. %u)", pass_samples, sample_chunk, pass_max_samples_per_pixel);
	rt_hip_adaptive_params p; // (what is wrong with the parameters is said before the context is looked at)
	if (const rt_hip_status st = resolve_adaptive("rt_hip_adaptive_update_device", params, whole_pass ? pass_samples : 0u, p))
		return st;
	if (!ctx || !d_accum || !d_pass_sum || !d_moments || !d_state || !d_rgba8_out)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_adaptive_update_device: NULL argument");
	if (!width || !height || width > max_frame_side || height > max_frame_side)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_adaptive_update_device: frame %ux%u (1 .. %u a side)", width, height, max_frame_side);
	const size_t pixels = static_cast<size_t>(width) * height;
	const struct
	{
		const void* ptr;
		size_t bytes;
		const char* name;
	} buffers[] = { { d_accum, pixels * 12u, "d_accum" }, { d_pass_sum, pixels * 12u, "d_pass_sum" }, { d_moments, pixels * 8u, "d_moments" }, { d_state, pixels * 4u, "d_state" },
					{ d_rgba8_out, pixels * 4u, "d_rgba8_out" }, { d_rgb_out, pixels * 12u, "d_rgb_out" }, { d_active_pixels, 4u, "d_active_pixels" } };
	for (size_t i = 0; i < sizeof buffers / sizeof buffers[0]; i++)
		for (size_t j = i + 1; j < sizeof buffers / sizeof buffers[0]; j++)
			if (buffers[i].ptr && buffers[j].ptr && buffers_overlap(buffers[i].ptr, buffers[i].bytes, buffers[j].ptr, buffers[j].bytes))
				return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_adaptive_update_device: %s overlaps %s (a pixel reads its neighbours' words)", buffers[i].name, buffers[j].name);
	try
	{
		RT_HIP_TRY(hipSetDevice(ctx->device)); // (a multi-GPU, rank or frame-group context: the root member, like the other device-level calls)
		return launch_update(ctx, width, height, pass_samples, first_pass != 0u, whole_pass != 0u, p, d_accum, d_pass_sum, d_moments, d_state, d_rgba8_out, d_rgb_out, d_active_pixels, static_cast<hipStream_t>(stream));
	}
	catch (const std::exception& e)
	{
		return fail(RT_HIP_RUNTIME_ERROR, "rt_hip_adaptive_update_device: %s", e.what());
	}
}

extern "C" rt_hip_status rt_hip_adaptive_pass_device(rt_hip_ctx* ctx,
														 uint32_t width,
														 uint32_t height,
														 uint64_t seed,
														 uint32_t flags,
														 uint32_t first_sample,
														 uint32_t n_samples,
														 const rt_hip_adaptive_params* params,
														 float* d_block,
														 uint32_t* d_rgba8,
														 float* d_rgb_f32,
														 uint32_t* d_active_pixels,
														 void* stream)
{
	if (first_sample % sample_chunk)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_adaptive_pass_device: first_sample %u is not a multiple of %u (a pass continues the chunk-wise fold of the pixel sums)", first_sample, sample_chunk);
	// a whole pass: whole chunks, and the passes before it were of its size; anything else is the short last pass, which judges nobody
	const bool whole_pass = n_samples && n_samples % sample_chunk == 0u && first_sample % n_samples == 0u;
	rt_hip_adaptive_params p;
	if (const rt_hip_status st = resolve_adaptive("rt_hip_adaptive_pass_device", params, whole_pass ? n_samples : 0u, p))
		return st;
	if (!ctx || !d_block || !d_rgba8)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_adaptive_pass_device: NULL argument");
	if (!width || !height || width > max_frame_side || height > max_frame_side)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_adaptive_pass_device: frame %ux%u (1 .. %u a side)", width, height, max_frame_side);
	if (const char* const refused = refused_adaptive_flag(flags))
		return fail(RT_HIP_UNSUPPORTED, "rt_hip_adaptive_pass_device: %s is not available for adaptive passes (0x%x): they take RT_HIP_FLAG_SM_MATERIALS, RT_HIP_FLAG_BVH, RT_HIP_FLAG_BVH_DEVICE_BUILD and RT_HIP_FLAG_STATS", refused, flags);
	if (ctx->multi || ctx->group || ctx->world != 1u)
		return fail(RT_HIP_UNSUPPORTED, "rt_hip_adaptive_pass_device: contexts from rt_hip_create only (adaptive passes trace the whole image: no multi-GPU, rank or frame-group context, no partition)");
	if (!ctx->have_scene)
		return fail(RT_HIP_NO_SCENE, "rt_hip_adaptive_pass_device: no scene uploaded");
	const uint32_t total = ctx->samples_per_pixel;
	if (total > pass_max_samples_per_pixel)
		return fail(RT_HIP_UNSUPPORTED, "rt_hip_adaptive_pass_device: %u samples per pixel: the samples' random windows alias beyond %u", total, pass_max_samples_per_pixel);
	if (!n_samples || first_sample >= total || n_samples > total - first_sample || (n_samples % sample_chunk && first_sample + n_samples != total))
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_adaptive_pass_device: samples [%u, %u + %u) are not whole chunks of %u within the scene's %u samples per pixel (the last pass alone may end on the sample count)", first_sample,
					first_sample, n_samples, sample_chunk, total);
	const size_t pixels = static_cast<size_t>(width) * height;
	if (buffers_overlap(d_block, pixels * block_words * 4u, d_rgba8, pixels * 4u) || (d_rgb_f32 && buffers_overlap(d_block, pixels * block_words * 4u, d_rgb_f32, pixels * 12u))
		|| (d_active_pixels && buffers_overlap(d_block, pixels * block_words * 4u, d_active_pixels, 4u)))
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_adaptive_pass_device: an output overlaps d_block");
	try
	{
		// (RT_HIP_FLAG_STATS asks for what this call keeps anyway, as rt_hip_render_pass_device does; which pixels were active only the
		// device knows: the update kernel counts them for the stats' primary_samples)
		return adaptive_pass(ctx, width, height, seed, flags, first_sample, n_samples, whole_pass, p, d_block, d_rgba8, d_rgb_f32, d_active_pixels, static_cast<hipStream_t>(stream), true, true);
	}
	catch (const std::exception& e)
	{
		return fail(RT_HIP_RUNTIME_ERROR, "rt_hip_adaptive_pass_device: %s", e.what());
	}
}

extern "C" rt_hip_status rt_hip_render_adaptive(rt_hip_ctx* ctx,
													const rt_hip_scene* scene,
													uint32_t* pixels_rgba8888,
													uint32_t width,
													uint32_t height,
													uint64_t seed,
													uint32_t flags,
													uint32_t pass_samples,
													const rt_hip_adaptive_params* params,
													float* rgb_f32,
													uint32_t* sample_counts,
													rt_hip_stats* stats,
													rt_hip_adaptive_info* out_info)
{
	const auto entered = std::chrono::steady_clock::now();
	const uint64_t pass_size = adaptive_pass_size(pass_samples);
	rt_hip_adaptive_params p; // (said before the context is looked at)
	if (const rt_hip_status st = resolve_adaptive("rt_hip_render_adaptive", params, pass_size, p))
		return st;
	if (!ctx || !scene || !pixels_rgba8888)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_render_adaptive: NULL argument");
	if (!width || !height || width > max_frame_side || height > max_frame_side)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_render_adaptive: frame %ux%u (1 .. %u a side)", width, height, max_frame_side);
	if (const rt_hip_status st = single_context_only("rt_hip_render_adaptive", ctx))
		return st;
	if (const char* const refused = refused_adaptive_flag(flags))
		return fail(RT_HIP_UNSUPPORTED, "rt_hip_render_adaptive: %s is not available for adaptive passes (0x%x): they take RT_HIP_FLAG_SM_MATERIALS, RT_HIP_FLAG_BVH, RT_HIP_FLAG_BVH_DEVICE_BUILD and RT_HIP_FLAG_STATS", refused, flags);
	if (!scene->samples_per_pixel || scene->samples_per_pixel > pass_max_samples_per_pixel)
		return fail(RT_HIP_UNSUPPORTED, "rt_hip_render_adaptive: %u samples per pixel (the cap: 1 .. %u, beyond which the samples' random windows alias)", scene->samples_per_pixel, pass_max_samples_per_pixel);
	if (pass_size > pass_max_samples_per_pixel)
		return fail(RT_HIP_UNSUPPORTED, "rt_hip_render_adaptive: a pass of %u samples", pass_samples);
	const size_t pixels = static_cast<size_t>(width) * height;
	const size_t frame_bytes = pixels * sizeof(uint32_t), block_bytes = pixels * block_words * sizeof(uint32_t);
	const bool keep_stats = stats || (flags & RT_HIP_FLAG_STATS);
	try
	{
		RT_HIP_TRY(hipSetDevice(ctx->device));
		track_frame_buffer(ctx, pixels_rgba8888, frame_bytes, false); // (a page-lock an earlier rt_hip_render took on the caller's buffer is dropped)

		scene_request request;
		if (const rt_hip_status st = resident_scene(ctx, scene, request))
			return st;

		adaptive_accumulation& a = ctx->adaptive;
		const adaptive_key wanted = make_adaptive_key(frame_key_of(request, scene, width, height, seed, flags & pass_frame_flags), p, static_cast<uint32_t>(pass_size));
		const adaptive_step step = next_adaptive_pass(a.state, wanted);
		if (step.restart)
			a.state = adaptive_state{};
		rt_hip_adaptive_info info{};
		info.samples_total = scene->samples_per_pixel;
		info.restarted = step.restart ? 1u : 0u;
		info.pixels = static_cast<uint32_t>(pixels);

		carried_frame frame(ctx, pixels_rgba8888, rgb_f32, pixels);
		if (const rt_hip_status st = frame.open("rt_hip_render_adaptive"))
			return st;
		const hipStream_t s = ctx->stream;
		// what lands on the host: the active word and the state words behind a pass; accum and state for a call on a complete accumulation
		const size_t landing_bytes = std::max(4u * pixels * sizeof(uint32_t), frame_bytes + sizeof(uint32_t));
		RT_HIP_TRY(a.staging.reserve(landing_bytes));

		if (!step.n_samples)
		{
			// A complete accumulation: nothing is launched.  The frame was kept on the host; the float mean is every pixel's running sum
			// over its own sample count — pixel_mean's division, correctly rounded on either side of the bus.
			if (a.frame.size() != pixels || a.block.bytes < block_bytes)
				return fail(RT_HIP_RUNTIME_ERROR, "rt_hip_render_adaptive: the finished frame was not kept");
			frame.delivery->carrier.copy(pixels_rgba8888, a.frame.data(), frame_bytes);
			if (rgb_f32 || sample_counts)
			{
				RT_HIP_TRY(hipMemcpyAsync(a.staging.ptr, a.block.ptr, 4u * pixels * sizeof(uint32_t), hipMemcpyDeviceToHost, s)); // accum, state
				RT_HIP_TRY(hipStreamSynchronize(s));
				const float* const sums = a.staging.as<float>();
				const uint32_t* const words = a.staging.as<uint32_t>() + 3u * pixels;
				for (size_t i = 0; i < pixels; i++)
				{
					const uint32_t n = adaptive::samples_of(words[i]);
					if (sample_counts)
						sample_counts[i] = n;
					if (rgb_f32)
						for (size_t c = 0; c < 3; c++)
							rgb_f32[i * 3 + c] = sums[i * 3 + c] / static_cast<float>(n);
				}
			}
			nothing_launched(ctx);
			info.samples_done = a.state.samples_done, info.passes = a.state.passes, info.active_pixels = a.state.active_pixels;
			info.samples_traced = a.state.samples_traced, info.complete = 1u;
			remember(info);
			if (out_info)
				*out_info = info;
			if (stats)
				*stats = ctx->stats;
			return ok();
		}

		RT_HIP_TRY(a.block.reserve(block_bytes)); // (grows only where an accumulation starts: the frame's size is part of its key)
		RT_HIP_TRY(a.active.reserve(sizeof(uint32_t)));
		if (!a.end)
			RT_HIP_TRY(hipEventCreate(&a.end));

		if (const rt_hip_status st = frame.begin())
			return st;
		// a pass that fails leaves the block in an unknown state: nothing is in flight from here until it has succeeded
		const adaptive_state before = a.state;
		a.state = adaptive_state{};
		if (const rt_hip_status st = adaptive_pass(ctx, width, height, seed, flags, step.first_sample, step.n_samples, step.whole_pass, p, a.block.as<float>(), frame.d_frame, frame.d_rgb, a.active.as<uint32_t>(), s, keep_stats))
			return st;
		frame.launched();
		if (keep_stats)
			RT_HIP_TRY(hipEventRecord(a.end, s));
		unsigned char* const landing = a.staging.as<unsigned char>();
		hipError_t e = hipMemcpyAsync(landing, a.active.ptr, sizeof(uint32_t), hipMemcpyDeviceToHost, s);
		if (e == hipSuccess && sample_counts)
			e = hipMemcpyAsync(landing + sizeof(uint32_t), view_of(a.block.as<float>(), pixels).state, frame_bytes, hipMemcpyDeviceToHost, s);
		if (const rt_hip_status st = frame.deliver(keep_stats ? a.end : nullptr, e))
			return st;
		uint32_t active_after = 0;
		std::memcpy(&active_after, landing, sizeof active_after);
		if (sample_counts)
		{
			const uint32_t* const words = reinterpret_cast<const uint32_t*>(landing + sizeof(uint32_t));
			for (size_t i = 0; i < pixels; i++)
				sample_counts[i] = adaptive::samples_of(words[i]);
		}

		const uint64_t traced_pixels = step.first_sample ? before.active_pixels : pixels; // the pixels that were active in this pass
		a.state = before;
		a.state.started = true;
		a.state.key = wanted;
		a.state.samples_done = step.first_sample + step.n_samples;
		a.state.active_pixels = active_after;
		a.state.passes = (step.restart ? 0u : before.passes) + 1u;
		a.state.samples_traced = (step.restart ? 0u : before.samples_traced) + traced_pixels * step.n_samples;
		const bool complete = adaptive_complete(scene->samples_per_pixel, a.state.samples_done, active_after);
		if (complete) // later calls deliver this frame again without a launch
			a.frame.assign(pixels_rgba8888, pixels_rgba8888 + pixels);
		info.samples_done = a.state.samples_done, info.passes = a.state.passes, info.active_pixels = active_after;
		info.samples_traced = a.state.samples_traced, info.complete = complete ? 1u : 0u;
		remember(info);
		if (out_info)
			*out_info = info;

		ctx->stats.primary_samples = traced_pixels * step.n_samples;
		if (const rt_hip_status st = frame.account(entered, stats))
			return st;
		if (stats)
			stats->render_ms = elapsed_or_zero(ctx->render_begin, a.end); // the traced pass and the update behind it
		return ok();
	}
	catch (const std::exception& e) // nothing may propagate through the C boundary
	{
		return fail(RT_HIP_RUNTIME_ERROR, "rt_hip_render_adaptive: %s", e.what());
	}
}
