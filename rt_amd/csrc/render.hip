// rt_amd/csrc/render.hip — one launch of the render kernels on a context (rt_hip_render_device), the work counters, and the
// single-GPU drop-in for renderer_interface::render (rt_hip_render; reference src/renderer.hpp:11,
// src/renderers/mg_ray_tracer.cpp:178-205).
#include "internal.hpp"

#include <algorithm>
#include <cstdio>
#include <exception>

using namespace rt_hip;

namespace
{
	// Is this "device" pointer page-locked host memory (a caller may hand rt_hip_render_device the device view of its own
	// registered buffer)?  Asked once per pointer: the answer of the last one is kept.
	bool is_host_memory(rt_hip_ctx* ctx, const void* pointer)
	{
		if (pointer != ctx->asked_pointer)
		{
			hipPointerAttribute_t attributes{};
			const hipError_t e = hipPointerGetAttributes(&attributes, pointer);
			if (e != hipSuccess)
				(void)hipGetLastError();
			ctx->asked_pointer = pointer;
			ctx->asked_pointer_is_host = e == hipSuccess && attributes.type == hipMemoryTypeHost;
		}
		return ctx->asked_pointer_is_host;
	}
}

extern "C" rt_hip_status rt_hip_render_device(rt_hip_ctx* ctx,
											  uint32_t width,
											  uint32_t height,
											  uint64_t seed,
											  uint32_t flags,
											  const rt_hip_partition* part,
											  uint32_t* d_rgba8,
											  float* d_rgb_f32,
											  void* stream)
{
	return render_device(ctx, width, height, seed, flags, part, d_rgba8, d_rgb_f32, stream, false, true, ctx && d_rgba8 && is_host_memory(ctx, d_rgba8), nullptr, true);
}

// one pass of a progressive frame at the device level (rt_hip.h): samples [first_sample, first_sample + n_samples) of the
// resident scene, folded onto the caller's accumulator
extern "C" rt_hip_status rt_hip_render_pass_device(rt_hip_ctx* ctx,
													   uint32_t width,
													   uint32_t height,
													   uint64_t seed,
													   uint32_t flags,
													   const rt_hip_partition* part,
													   uint32_t first_sample,
													   uint32_t n_samples,
													   float* d_accum,
													   uint32_t* d_rgba8,
													   float* d_rgb_f32,
													   void* stream)
{
	if (first_sample % sample_chunk)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_render_pass_device: first_sample %u is not a multiple of %u (a pass continues the chunk-wise fold of the pixel sums)", first_sample, sample_chunk);
	if (!ctx || !d_accum || !d_rgba8)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_render_pass_device: NULL argument");
	if (const char* const refused = refused_pass_flag(flags))
		return fail(RT_HIP_UNSUPPORTED, "rt_hip_render_pass_device: %s is not available for passes (0x%x): they take RT_HIP_FLAG_SM_MATERIALS, RT_HIP_FLAG_BVH, RT_HIP_FLAG_BVH_DEVICE_BUILD and RT_HIP_FLAG_STATS", refused, flags);
	if (!ctx->have_scene)
		return fail(RT_HIP_NO_SCENE, "rt_hip_render_pass_device: no scene uploaded");
	const uint32_t total = ctx->samples_per_pixel;
	if (total > pass_max_samples_per_pixel)
		return fail(RT_HIP_UNSUPPORTED, "rt_hip_render_pass_device: %u samples per pixel: the samples' random windows alias beyond %u", total, pass_max_samples_per_pixel);
	if (!n_samples || first_sample >= total || n_samples > total - first_sample || (n_samples % sample_chunk && first_sample + n_samples != total))
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_render_pass_device: samples [%u, %u + %u) are not whole chunks of %u within the scene's %u samples per pixel (the last pass alone may end on the sample count)", first_sample,
					first_sample, n_samples, sample_chunk, total);
	const render_pass pass = { first_sample, n_samples, d_accum };
	// (RT_HIP_FLAG_STATS asks for what this call keeps anyway, as rt_hip_render_device does: it is not the launch's)
	return render_device(ctx, width, height, seed, flags & pass_flag_mask, part, d_rgba8, d_rgb_f32, stream, false, true, is_host_memory(ctx, d_rgba8), &pass);
}

namespace rt_hip
{
rt_hip_status render_device(rt_hip_ctx* ctx, uint32_t width, uint32_t height, uint64_t seed, uint32_t flags, const rt_hip_partition* part, uint32_t* d_rgba8, float* d_rgb_f32, void* stream, bool whole_frame_buffers, bool keep_stats, bool host_frame,
							const render_pass* pass, bool sky_band)
{
	if (!ctx || !d_rgba8)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_render_device: NULL argument");
	const render_check checked = check_render_request(width, height, flags, part); // flag combinations, the frame's size, the partition
	if (checked.status)
		return fail(checked.status, "%s", checked.message);
	flags = checked.flags; // (the launch's: without the BVH bits for the preview, without the builder's)
	if (!ctx->have_scene)
		return fail(RT_HIP_NO_SCENE, "rt_hip_render_device: no scene uploaded");
	// RT_HIP_FLAG_EMISSION: the frame is checked against the context's table before anything is enqueued (the preview has dropped the flag)
	if (flags & RT_HIP_FLAG_EMISSION)
	{
		const light_check table = check_emission_table("rt_hip_render_device", ctx->have_emission, ctx->emission_rows, ctx->scene.n_materials);
		if (table.status)
			return fail(table.status, "%s", table.message);
	}
	RT_HIP_TRY(hipSetDevice(ctx->device));
	const hipStream_t s = static_cast<hipStream_t>(stream);
	// A context serialises its launches: they share the work counters, the tile queue's head and the timing events.  Work
	// on one stream is ordered by the stream; a caller that moves to ANOTHER stream first waits for the old one to drain
	// (a rare event: rt_hip_render always uses the context's own stream).
	if (ctx->launched && ctx->last_stream != s)
		RT_HIP_TRY(hipStreamSynchronize(ctx->last_stream));

	frame_request wanted{};
	wanted.width = width, wanted.height = height, wanted.partition = checked.partition;
	// (a pass: the kernels' sample count is the one AFTER the pass — what its fold divides by, and where its last chunk ends)
	wanted.samples_per_pixel = pass ? pass->first_sample + pass->n_samples : ctx->samples_per_pixel, wanted.max_bounces = ctx->max_bounces;
	wanted.seed = seed, wanted.whole_frame_buffers = whole_frame_buffers;
	std::copy(ctx->inverse_view_projection, ctx->inverse_view_projection + 16, wanted.inverse_view_projection);
	frame_params f = make_frame_params(wanted);
	// RT_HIP_FLAG_THIN_LENS: the frame is checked against the context's lens and its own camera before anything is enqueued (the preview has
	// dropped the flag).  With an aperture of 0 the frame is the flag-less frame in every respect: the flag ends here.
	if (flags & RT_HIP_FLAG_THIN_LENS)
	{
		const lens_check lens = check_lens_frame("rt_hip_render_device", ctx->have_lens, f);
		if (lens.status)
			return fail(lens.status, "%s", lens.message);
		if (!(ctx->lens.aperture_radius > 0.0f))
			flags &= ~static_cast<uint32_t>(RT_HIP_FLAG_THIN_LENS);
	}

	// every decision of the launch is made here, once: the buffers below are prepared from the plan the launch code then follows
	launch_plan plan{}; // (the preview: nothing to plan)
	rolling_buffers rolling;
	uint32_t band_rows = 0, band_variant = RT_HIP_KERNEL_NONE; // the sky band's rows (0: none) and the kernel variant the frame reports with one
	if (!(flags & RT_HIP_FLAG_PREVIEW))
	{
		launch_request request{};
		request.n_spheres = ctx->scene.n_spheres, request.n_planes = ctx->scene.n_planes, request.planes_tame = ctx->scene.planes_tame != 0;
		request.width = width, request.local_rows = f.local_rows, request.samples_per_pixel = pass ? ctx->samples_per_pixel : f.samples_per_pixel;
		if (pass)
			request.pass_first_sample = pass->first_sample, request.pass_samples = pass->n_samples, request.adaptive = pass->adaptive;
		request.camera = camera_form_of(f);
		request.flags = flags, request.host_frame = host_frame, request.fast_arithmetic = (flags & RT_HIP_FLAG_FAST) != 0;
		request.n_boxes = ctx->scene.n_boxes;
		request.n_lights = (flags & RT_HIP_FLAG_EMISSION) ? ctx->emission_lights : 0u;
		// RT_HIP_FLAG_DIRECT_LIGHT: the plan looks at how many SAMPLED lights the resident scene has under the table, and the list's builder counts
		// them (scene.hip: the light variant of the tables, built if missing or stale — a table build like the hierarchy's, nothing is enqueued)
		if ((flags & RT_HIP_FLAG_DIRECT_LIGHT) && request.n_lights != 0u && !pass)
		{
			if (const rt_hip_status st = ensure_light_tables(ctx))
				return st;
			RT_HIP_TRY(hipSetDevice(ctx->device));
			request.n_sampled_lights = ctx->sampled_lights;
		}
		request.lens_aperture = (flags & RT_HIP_FLAG_THIN_LENS) ? ctx->lens.aperture_radius : 0.0f;
		request.lds_limit = ctx->workgroup_lds_bytes;
		plan = plan_launch(request);
		// the refusals of the plan come before anything is enqueued — the hierarchy's build included
		if (plan.refusal[0]) // (traced boxes beyond what the box builds hold, or tables and chunk sums beyond a workgroup's LDS on this device: nothing is launched)
			return fail(RT_HIP_UNSUPPORTED, "rt_hip_render_device: %s", plan.refusal);
		// small scenes: a pixel's chunk sums (one per 16 samples) are parked in LDS until the pixel is complete
		if (pass && plan.slot_bytes > max_slot_bytes)
			return fail(RT_HIP_UNSUPPORTED, "rt_hip_render_pass_device: a pass of %u samples is more than the kernels hold chunk sums for (4096 per pass; the frame's samples_per_pixel has no such limit)", pass->n_samples);
		if (plan.slot_bytes > max_slot_bytes)
			return fail(RT_HIP_UNSUPPORTED, "rt_hip_render_device: %u samples per pixel are more than the kernels hold chunk sums for (4096; the reference clamps to 1000, src/scene.cpp:544)", f.samples_per_pixel);
		// the hierarchy kernel: under RT_HIP_FLAG_BVH with the builder the call names; a pass, or a frame with traced boxes, of a scene of the streamed
		// kernel's size, and every frame of RT_HIP_FLAG_BOX_BVH, go through it flag or no flag (plan_launch), on the host's tree
		if (plan.build.scan == scan_bvh)
		{
			if (const rt_hip_status st = ensure_bvh(ctx, (flags & RT_HIP_FLAG_BVH) ? checked.bvh_device_build : false, s, keep_stats))
				return st;
			RT_HIP_TRY(hipSetDevice(ctx->device));
			rolling.bvh = ctx->bvh_descriptor;
		}
		if (plan.build.box_tree) // RT_HIP_FLAG_BOX_BVH: the box hierarchy's descriptor travels behind (a copy of) the sphere hierarchy's
		{
			if (const rt_hip_status st = ensure_box_bvh(ctx, s))
				return st;
			rolling.bvh = ctx->box_bvh_block.as<const device_bvh>();
		}
		if (pass)
			rolling.accum = pass->d_accum;
		if (plan.build.lights) // RT_HIP_FLAG_EMISSION with at least one light: the light variant of the per-primitive tables, built if missing or stale
		{
			if (const rt_hip_status st = ensure_light_tables(ctx))
				return st;
			RT_HIP_TRY(hipSetDevice(ctx->device));
		}
		// big scenes: they meet in HBM, 16 bytes per chunk (or per sample) of this rank's rows
		if (plan.item_sums_bytes > ctx->item_sums.bytes && plan.queue.halves && plan.big_scene && ctx->item_sums.reserve(plan.item_sums_bytes) != hipSuccess)
		{
			// no room for a slot per SAMPLE (up to 8 GiB): whole chunks need a sixteenth of it — the one launch that is planned twice
			(void)hipGetLastError();
			request.flags |= RT_HIP_FLAG_FORCE_WHOLE_CHUNKS;
			request.flags &= ~static_cast<uint32_t>(RT_HIP_FLAG_FORCE_HALF_CHUNKS);
			plan = plan_launch(request);
		}
		if (plan.item_sums_bytes > (64ull << 30))
			return fail(RT_HIP_UNSUPPORTED, "%s: %ux%u at %u samples per pixel needs %zu GiB for the chunk sums of a scene of this size", pass ? "rt_hip_render_pass_device" : "rt_hip_render_device", width, height, f.samples_per_pixel, plan.item_sums_bytes >> 30);
		if (plan.item_sums_bytes)
		{
			RT_HIP_TRY(ctx->item_sums.reserve(plan.item_sums_bytes));
			RT_HIP_TRY(ctx->pixel_done.reserve(plan.pixel_done_bytes));
			// The arrival counters start every launch at zero — set here, on the launch's own stream, not left behind by the
			// previous launch: a launch that did not run to its end (a failed or aborted one) must not cost later frames
			// their pixels.  (8 MB at 1080p in front of a launch of milliseconds to seconds.)
			RT_HIP_TRY(hipMemsetAsync(ctx->pixel_done.ptr, 0, plan.pixel_done_bytes, s));
			rolling.item_sums = ctx->item_sums.as<unsigned long long>();
			rolling.pixel_done = ctx->pixel_done.as<uint32_t>();
		}
		// The sky band (sky_band.hpp): the rows from the top of the image that provably see nothing go to a scene-free
		// kernel of their own, and the plan's kernel is launched over the rows below — planned as any shorter launch is.  The rule
		// is asked once per (scene, camera, size, flags): an unmoved camera's further frames pay a comparison.  Only the two callers that
		// render one whole frame in one launch offer a band (`sky_band`), and never for a pass: a pass build reads its first chunk where
		// the other tile-per-wave builds read the band's height, and its accumulator is no business of the band's kernel.
		// (A lens frame never takes the band: the band's proof is about rays that leave the eye.)
		if (plan.build.lens)
			put_lens_words(f, make_lens_words(f, ctx->inverse_view_projection, ctx->lens)); // (the ten words, where only the homogeneous form reads)
		if (ctx->sky_band_enabled && sky_band && !pass && !plan.build.lens)
		{
			frame_params asked = f;
			asked.frame_key_a = asked.frame_key_b = 0u; // (the seed does not move a ray)
			auto& last = ctx->sky_band_asked;
			if (!(last.valid && last.scene_uploads == ctx->scene_uploads && last.flags == flags && last.scan == plan.build.scan && std::memcmp(&last.frame, &asked, sizeof(asked)) == 0))
			{
				const sky_band_request rule = { ctx->sphere_table.data(), ctx->scene.n_spheres, ctx->scene.n_planes, flags, false, false, plan.build.scan, &f };
				last.rows = sky_band_rows(rule);
				last.valid = true, last.scene_uploads = ctx->scene_uploads, last.flags = flags, last.scan = plan.build.scan, last.frame = asked;
			}
			if (last.rows)
			{
				request.local_rows = f.local_rows - last.rows;
				const launch_plan below = plan_launch(request);
				const bool tile_per_wave = below.build.scan > 0 || below.build.scan == scan_resident;
				if (!below.refusal[0] && below.slot_bytes <= max_slot_bytes && !below.item_sums_bytes && tile_per_wave)
				{
					band_rows = last.rows;
					band_variant = plan.variant; // (what the frame reports: the kernel of its scene, also where every row is sky)
					plan = below;
				}
			}
		}
		if (ctx->sky_band_log)
			std::fprintf(stderr, "rt_hip sky band: rows %u of %u (%ux%u, flags 0x%x)\n", band_rows, height, width, height, flags);
	}
	device_counters* const counters = ctx->counters.as<device_counters>();
	if (keep_stats)
	{
		RT_HIP_TRY(hipMemsetAsync(counters, 0, sizeof(device_counters), s));
		RT_HIP_TRY(hipEventRecord(ctx->render_begin, s));
	}
	else if (plan.big_scene) // the persistent big-scene kernels draw items from a sequence whose head must start at 0
		RT_HIP_TRY(hipMemsetAsync(&counters->next_item, 0, sizeof(counters->next_item), s)); // (seconds-long launches: not launch-bound)
	uint32_t variant = RT_HIP_KERNEL_PREVIEW;
	// (inside the event pair that yields render_ms, in front of the scene's kernel; an experiment build with RT_HIP_SKY_BAND_LAST puts it
	// behind instead: measured)
	const auto launch_band = [&]()
	{
		frame_params band = f;
		band.local_rows = band_rows;
		launch_sky_band(band, d_rgba8, d_rgb_f32, counters, s);
	};
#ifndef RT_HIP_SKY_BAND_LAST
	if (band_rows)
		launch_band();
#endif
	if (flags & RT_HIP_FLAG_PREVIEW)
		launch_preview(f, ctx->scene, d_rgba8, d_rgb_f32, counters, s);
	else if (flags & RT_HIP_FLAG_FAST)
		variant = launch_render_fast({ f, ctx->scene, ctx->small, plan, d_rgba8, d_rgb_f32, counters, rolling, ctx->compute_units, ctx->cache, s });
	else if (plan.build.lights)
	{
		// the light builds read the SAME device_scene words: a copy whose four per-primitive shading / scatter pointers point at the light variant
		device_scene lit = ctx->scene;
		lit.primitive_shading = ctx->light_shading, lit.primitive_scatter = ctx->light_scatter;
		lit.primitive_shading_sm = ctx->light_shading_sm, lit.primitive_scatter_sm = ctx->light_scatter_sm;
		if (plan.build.direct) // (the scatter tables that tell a sampled light from a light that counts on hit; the list lies in front of light_shading)
			lit.primitive_scatter = ctx->light_scatter_direct, lit.primitive_scatter_sm = ctx->light_scatter_sm_direct;
		variant = launch_render({ f, lit, (flags & RT_HIP_FLAG_SM_MATERIALS) ? ctx->small_sm : ctx->small, plan, d_rgba8, d_rgb_f32, counters, rolling, ctx->compute_units, ctx->cache, s });
	}
	else
		variant = launch_render({ f, ctx->scene, (flags & RT_HIP_FLAG_SM_MATERIALS) ? ctx->small_sm : ctx->small, plan, d_rgba8, d_rgb_f32, counters, rolling, ctx->compute_units, ctx->cache, s, band_rows }); // (below a band: the plan's grid covers rows [band_rows, height), the kernel is told the first)
#ifdef RT_HIP_SKY_BAND_LAST
	if (band_rows)
		launch_band();
#endif
	if (band_rows)
		variant = band_variant;
	RT_HIP_TRY(hipGetLastError());
	ctx->launched = true;
	ctx->last_stream = s;
	if (keep_stats)
	{
		RT_HIP_TRY(hipEventRecord(ctx->render_end, s));
		// the counters follow the kernel to the host on the same stream: reading them later costs no transfer of its own
		RT_HIP_TRY(hipMemcpyAsync(ctx->counters_host, counters, sizeof(device_counters), hipMemcpyDeviceToHost, s));
		RT_HIP_TRY(hipEventRecord(ctx->counters_copied, s));
	}
	ctx->render_recorded = keep_stats;
	ctx->adaptive.traced_pass_samples = 0; // (rt_hip_adaptive_pass_device sets it behind its update)
	ctx->stats.kernel_variant = variant;
	ctx->stats.primary_samples = static_cast<uint64_t>(f.local_rows) * width * ((flags & RT_HIP_FLAG_PREVIEW) ? 1u : (pass ? pass->n_samples : f.samples_per_pixel));
	if (!keep_stats) // the counters of this frame were not kept: nothing stale may be reported for it
	{
		ctx->stats.render_ms = 0.0f;
		ctx->stats.segments = ctx->stats.sphere_tests = ctx->stats.plane_tests = 0;
	}
	return ok();
}
}

extern "C" rt_hip_status rt_hip_assemble_device(rt_hip_ctx* ctx,
												uint32_t width,
												uint32_t height,
												uint32_t world,
												uint32_t stripe_rows,
												const uint32_t* d_gathered,
												uint32_t* d_frame,
												void* stream)
{
	if (!ctx || !d_gathered || !d_frame)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_assemble_device: NULL argument");
	if (!width || !height || !world || !stripe_rows)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_assemble_device: zero size");
	RT_HIP_TRY(hipSetDevice(ctx->device));
	const rt_hip_partition p = { 0, world, stripe_rows };
	uint32_t padded = 0;
	if (const rt_hip_status st = rt_hip_padded_local_rows(height, &p, &padded))
		return st;
	launch_assemble(width, height, world, stripe_rows, padded, d_gathered, d_frame, 0u, false, static_cast<hipStream_t>(stream));
	RT_HIP_TRY(hipGetLastError());
	return ok();
}

namespace rt_hip
{
	// synchronise with the member's last launch and read its counters into member->stats
	rt_hip_status fetch_member_stats(rt_hip_ctx* ctx)
	{
		RT_HIP_TRY(hipSetDevice(ctx->device));
		if (ctx->render_recorded)
		{
			RT_HIP_TRY(hipEventSynchronize(ctx->counters_copied));
			float ms = 0.0f;
			RT_HIP_TRY(hipEventElapsedTime(&ms, ctx->render_begin, ctx->render_end));
			ctx->stats.render_ms = ms;
			uint64_t segments = 0;
			for (const unsigned long long part : ctx->counters_host->segments)
				segments += part;
			ctx->stats.segments = segments;
			ctx->stats.sphere_tests = segments * ctx->scene.n_spheres;
			ctx->stats.plane_tests = segments * ctx->scene.n_planes;
			// a device-level adaptive pass: the pixels that were active, counted by the update kernel, x the pass's samples
			if (ctx->adaptive.traced_pass_samples)
				ctx->stats.primary_samples = static_cast<uint64_t>(*ctx->adaptive.traced.as<uint32_t>()) * ctx->adaptive.traced_pass_samples;
#ifdef RT_HIP_BVH_CHECK // (experiment builds: tools/bvh_sweep.py --check reads this line)
			std::fprintf(stderr, "bvh_check: %llu queries, %llu disagreements\n", ctx->counters_host->bvh_checked, ctx->counters_host->bvh_disagreements);
#endif
		}
		return ok();
	}
}

namespace rt_hip
{
	rt_hip_stats stats_of_group_rank(const rt_hip_ctx* ctx, uint32_t rank)
	{
		const frame_group_rank& line = ctx->group->block->ranks[rank];
		rt_hip_stats out{};
		out.primary_samples = line.primary_samples;
		out.segments = line.segments;
		out.sphere_tests = line.sphere_tests;
		out.plane_tests = line.plane_tests;
		out.render_ms = line.render_ms;
		out.upload_ms = line.upload_ms;
		out.kernel_variant = line.kernel_variant;
		return out;
	}

	// whole-frame counters of a frame group: counts summed over the ranks, times the slowest rank's
	void sum_group_stats(const rt_hip_ctx* ctx, rt_hip_stats* out)
	{
		for (uint32_t r = 0; r < ctx->world; r++)
		{
			if (r == ctx->first_rank)
				continue;
			const rt_hip_stats other = stats_of_group_rank(ctx, r);
			out->primary_samples += other.primary_samples;
			out->segments += other.segments;
			out->sphere_tests += other.sphere_tests;
			out->plane_tests += other.plane_tests;
			out->render_ms = std::max(out->render_ms, other.render_ms);
			out->upload_ms = std::max(out->upload_ms, other.upload_ms);
		}
	}
}

extern "C" rt_hip_status rt_hip_stats_fetch(rt_hip_ctx* ctx, rt_hip_stats* out_stats)
{
	if (!ctx || !out_stats)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_stats_fetch: NULL argument");
	if (const rt_hip_status st = fetch_member_stats(ctx))
		return st;
	*out_stats = ctx->stats;
	if (ctx->group) // the other ranks' shares are in the group's block (valid between two frames)
		sum_group_stats(ctx, out_stats);
	// several GPUs: the frame's counts are the sum over the members' shares, its kernel time the slowest member's
	for (rt_hip_ctx* member : ctx->peers)
	{
		if (const rt_hip_status st = fetch_member_stats(member))
			return st;
		out_stats->primary_samples += member->stats.primary_samples;
		out_stats->segments += member->stats.segments;
		out_stats->sphere_tests += member->stats.sphere_tests;
		out_stats->plane_tests += member->stats.plane_tests;
		out_stats->render_ms = std::max(out_stats->render_ms, member->stats.render_ms);
		out_stats->upload_ms = std::max(out_stats->upload_ms, member->stats.upload_ms);
	}
	if (!ctx->peers.empty())
		RT_HIP_TRY(hipSetDevice(ctx->device));
	return ok();
}

extern "C" rt_hip_status rt_hip_member_stats(rt_hip_ctx* ctx, int rank, rt_hip_stats* out_stats)
{
	if (ctx && ctx->group && out_stats && rank >= 0 && rank < static_cast<int>(ctx->world))
	{
		*out_stats = stats_of_group_rank(ctx, static_cast<uint32_t>(rank)); // (that rank's share of the most recent frame that kept stats)
		return ok();
	}
	rt_hip_ctx* member = member_of(ctx, rank);
	if (!member || !out_stats)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_member_stats: invalid argument");
	if (const rt_hip_status st = fetch_member_stats(member))
		return st;
	*out_stats = member->stats;
	RT_HIP_TRY(hipSetDevice(ctx->device));
	return ok();
}

extern "C" rt_hip_status rt_hip_phases_fetch(rt_hip_ctx* ctx, rt_hip_phases* out_phases)
{
	if (!ctx || !out_phases)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_phases_fetch: NULL argument");
	*out_phases = ctx->phases;
	return ok();
}

extern "C" rt_hip_status rt_hip_render(rt_hip_ctx* ctx,
									   const rt_hip_scene* scene,
									   uint32_t* pixels_rgba8888,
									   uint32_t width,
									   uint32_t height,
									   uint64_t seed,
									   uint32_t flags,
									   float* rgb_f32,
									   rt_hip_stats* stats)
{
	const auto entered = std::chrono::steady_clock::now();
	if (!ctx || !scene || (!pixels_rgba8888 && !(ctx->multi && ctx->first_rank != 0) && !ctx->group))
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_render: NULL argument");
	if (!width || !height)
		return fail(RT_HIP_INVALID_ARGUMENT, "rt_hip_render: empty frame %ux%u", width, height);
	if (flags & ~(render_flag_mask | static_cast<uint32_t>(RT_HIP_FLAG_PERSISTENT_FRAME | RT_HIP_FLAG_STATS)))
		return fail(RT_HIP_UNSUPPORTED, "rt_hip_render: unknown flag bits 0x%x", flags);
	const size_t pixels = static_cast<size_t>(width) * height;
	const size_t frame_bytes = pixels * sizeof(uint32_t);
	const bool keep_stats = stats || (flags & RT_HIP_FLAG_STATS);
	try
	{
		RT_HIP_TRY(hipSetDevice(ctx->device));
		if (ctx->group)
			return render_group(ctx, scene, pixels_rgba8888, width, height, seed, flags, rgb_f32, stats, entered);
		if (pixels_rgba8888 && ctx->multi && ctx->direct_frame && ctx->peers.size() + 1 == ctx->world)
		{
			std::vector<int> nodes(1, ctx->numa_node); // every member stores its own stripes: each stripe on its member's node
			for (const rt_hip_ctx* member : ctx->peers)
				nodes.push_back(member->numa_node);
			track_frame_buffer(ctx, pixels_rgba8888, frame_bytes, (flags & RT_HIP_FLAG_PERSISTENT_FRAME) != 0, true, &nodes, width, height);
		}
		else if (pixels_rgba8888)
			track_frame_buffer(ctx, pixels_rgba8888, frame_bytes, (flags & RT_HIP_FLAG_PERSISTENT_FRAME) != 0);
		if (ctx->multi)
			return render_multi(ctx, scene, pixels_rgba8888, width, height, seed, flags, rgb_f32, stats, entered);

		scene_request request;
		if (const rt_hip_status st = resident_scene(ctx, scene, request))
			return st;
		// Where the kernel stores its finished pixels (4 bytes per pixel over PCIe while the rest of the frame is still being
		// traced): the caller's own buffer if it is page-locked and mapped (RT_HIP_FLAG_PERSISTENT_FRAME), else the module's
		// own page-locked frame, from which the carrier's threads take them on into the caller's buffer (frame.hip).
		uint32_t* direct = nullptr;
		if (ctx->pinned_frame)
		{
			void* device_view = nullptr;
			if (hipHostGetDevicePointer(&device_view, pixels_rgba8888, 0) == hipSuccess && device_view)
				direct = static_cast<uint32_t*>(device_view);
			else
				(void)hipGetLastError();
		}
		carried_frame frame(ctx, pixels_rgba8888, rgb_f32, pixels);
		if (const rt_hip_status st = frame.open("rt_hip_render"))
			return st;
		if (const rt_hip_status st = frame.begin(direct))
			return st;
		if (const rt_hip_status st = render_device(ctx, width, height, seed, flags & render_flag_mask, nullptr, frame.d_frame, frame.d_rgb, ctx->stream, false, keep_stats, true, nullptr, true))
			return st;
		frame.launched();
		if (const rt_hip_status st = frame.deliver(keep_stats ? ctx->render_end : nullptr))
			return st;
		return frame.account(entered, stats);
	}
	catch (const std::exception& e) // nothing may propagate through the C boundary
	{
		return fail(RT_HIP_RUNTIME_ERROR, "rt_hip_render: %s", e.what());
	}
}
