// rt_amd/csrc/launch_plan.cpp — the launch policy of the render kernels (launch_plan.hpp): host-only, plain C++17.
#include "launch_plan.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>

namespace rt_hip
{
	uint32_t choose_kernel(uint32_t n_spheres, uint32_t n_planes, bool planes_tame, uint32_t flags, uint32_t samples_per_pixel, bool perspective, uint64_t pixels)
	{
		const uint32_t primitives = n_spheres + n_planes;
		if (flags & RT_HIP_FLAG_BVH) // (check_render_request refuses it with the FORCE_ flags; render.hip builds the hierarchy first)
			return RT_HIP_KERNEL_BVH;
		if (flags & RT_HIP_FLAG_FORCE_STREAMED)
			return RT_HIP_KERNEL_STREAMED;
		if (flags & RT_HIP_FLAG_FORCE_TILED)
			return RT_HIP_KERNEL_TILED;
		// up to 8 primitives: at least one sphere, at most three planes (round 4: neither a plane nor a camera whose w varies
		// over the frame pushes a scene off this kernel any more)
		// ... through a camera with an eye (`perspective`: the pinhole or the plain eye form; the scalar-register kernels are built for those)
		// ... and planes whose normals are of ordinary size (device_scene::planes_tame)
		if (!(flags & RT_HIP_FLAG_FORCE_RESIDENT) && perspective && n_spheres >= 1 && n_planes <= scalar_max_planes && primitives <= scalar_max_spheres && (n_planes == 0 || planes_tame))
			return RT_HIP_KERNEL_SMALL;
		// The LDS-resident kernel (one tile per wave) up to streamed_from_primitives (launch_plan.hpp has the measurements), or whatever
		// its LDS can hold when forced; beyond that a trip is a long scan and the rolling hand-out of the big-scene kernels wins.
		const uint32_t staged = (n_spheres < resident_scalar_scan_from ? n_spheres : 0u) + n_planes; // what the resident kernel keeps in LDS
		// (Scenes beyond its LDS capacity only in frames that fill the device — 4M samples, 64 for every lane it holds: in a small
		// frame of a big scene every wave is a sparse one, and the streamed kernel scans those with all 64 lanes per ray.)
		const bool fits = primitives <= resident_max_primitives || (primitives <= streamed_from_primitives && pixels * samples_per_pixel >= (1ull << 22));
		if (staged <= resident_max_primitives && ((flags & RT_HIP_FLAG_FORCE_RESIDENT) || fits))
			return RT_HIP_KERNEL_RESIDENT;
		// Big scenes: the scalar-streamed kernel (no staging, no barriers).  Rounds 1-2 chose the LDS-tiled kernel below
		// 32 samples per pixel, where it was 2 % ahead; since the group prefetch, the cooperative scan of sparse waves and
		// the one-sample items the streamed kernel is 10-30 % ahead at every sample count from 1 to 24 and every size from
		// 1 100 to 100 000 spheres (profiles/r03/tiled_vs_streamed.txt).  The tiled kernel stays behind its flag.
		(void)samples_per_pixel;
		return RT_HIP_KERNEL_STREAMED;
	}

	namespace
	{
		// The frame as tiles of queue.pixels_log2 pixels, queue.tile_w_log2 of them in a row.  tiles_y is the launch grid's y dimension
		// (plan_launch), which holds at most max_grid_y workgroups: where the shape asked for would give more tile rows — a page-locked
		// frame's one-row tiles in a frame of more than 65535 rows — the next taller shape of the same pixel count is taken.  A tile holds
		// at least four pixels and a frame at most 2 x max_grid_y rows (check_render_request), so one step suffices; the loop says the rule,
		// not the count.  (The rolling kernels' 1 x 1 "tiles" are not launched as a grid: nothing to lower, grid_y is 1.)
		void cut_tiles(queue_params& q, uint32_t width, uint32_t local_rows)
		{
			constexpr uint32_t max_grid_y = 65535u;
			for (;;)
			{
				const uint32_t tile_w = 1u << q.tile_w_log2, tile_h = (1u << q.pixels_log2) >> q.tile_w_log2;
				q.tiles_x = (width + tile_w - 1u) / tile_w;
				q.tiles_y = (local_rows + tile_h - 1u) / tile_h;
				if (q.tiles_y <= max_grid_y || q.tile_w_log2 == 0u)
					return;
				q.tile_w_log2--;
			}
		}
	}

	queue_params choose_queue(uint32_t samples_per_pixel, uint32_t width, uint32_t local_rows, bool big_scene, bool host_frame, int half_chunks, uint32_t primitives, bool sparse_launch)
	{
		queue_params q{};
		q.chunks = (samples_per_pixel + sample_chunk - 1u) / sample_chunk; // K chunks per pixel
		uint32_t pixels_log2;
		if (big_scene)
		{
			// rolling items: no tiles at all (the fields below describe the frame as 1 x 1 tiles and are not used); a wave
			// draws 8 items at a time, one block ahead — small enough that a wave sits on at most 15 reserved items when
			// the sequence runs dry, large enough that the counter sees one atomic per wave every few trips
			pixels_log2 = 0;
			q.block_items = 8u;
			q.lane_cap = 64u;
			q.sparse_rays = sparse_wave_rays;
			// Sub-chunk items.  A trip of a big-scene wave costs the same with one lane holding a ray as with 64, and from the
			// moment the launch-wide sequence runs dry every lane still owes the rest of its item: with whole chunks the
			// last 10 % of config 5's launch ran on thinning waves (4.9 % of all wave-time after the waves' retirement alone,
			// profiles/r03/config5_streamed/wave_tail_items_sparse.txt), and its 8-way share — 2.6 chunks per lane — took
			// twice its share of the time.  Items may be ANY run of consecutive samples if every sample's VALUE is handed
			// over instead of a chunk's sum (16 bytes per sample through HBM: nothing next to a scan of the scene per path
			// segment) and the lane that brings a pixel's last item adds them up as the contract says.  How small: every item
			// costs an arrival (an atomic in HBM: the device does ~0.66 G of them per second, profiles/r03/item_sweep.txt),
			// which stays in the shadow of the tracing while samples-per-item x primitives >= 8192 — one sample per item from
			// 8192 primitives upwards, eight at 1025.  Measured: config 5 5.55 -> 5.10 s, its 1/8 share 1203 -> 636 ms;
			// 30 000 x 64 spp 1756 -> 1616; 10 000 x 32 spp 276 -> 244; 2 000 x 64 spp 96.4 -> 90.5; 1 025 x 64 spp 49.7 -> 47.1.
			q.item_samples = sample_chunk;
			if (half_chunks && samples_per_pixel > 1u && primitives)
			{
				uint32_t smallest = 1u;
				while (smallest < sample_chunk && static_cast<uint64_t>(smallest) * primitives < 8192u)
					smallest *= 2u;
				// (a sample's slot is 16 bytes: frames whose samples would need more than 8 GiB keep whole chunks)
				if (static_cast<uint64_t>(width) * local_rows * samples_per_pixel * 16u <= (8ull << 30))
					q.item_samples = smallest;
				if (half_chunks == 2 && q.item_samples == sample_chunk)
					q.item_samples = sample_chunk / 2u;
#ifdef RT_HIP_QUEUE_KNOBS
				if (const char* knob = std::getenv("RT_HIP_ITEM_SAMPLES")) // experiment builds only (tools/gpu_item_sweep.py)
					q.item_samples = static_cast<uint32_t>(std::atoi(knob));
#endif
				q.halves = q.item_samples < sample_chunk ? 1u : 0u;
#ifdef RT_HIP_QUEUE_KNOBS
				if (const char* knob = std::getenv("RT_HIP_BLOCK_ITEMS"))
					q.block_items = static_cast<uint32_t>(std::atoi(knob));
#endif
			}
			// Sparse launches of the streamed kernel.  A trip costs one sequential scan of the scene whether the wave holds 64
			// rays or one; the cooperative scan (scan_spheres_together) costs a wave about 1/40 of that PER RAY.  At the end of a
			// full launch, where the device is busy, it pays up to 8 rays (sparse_wave_rays: an A/B of round 3); in a launch
			// that cannot fill the device at all — fewer work items than 32 per wave it can hold — it pays all the way:
			// the launch is spread THIN, every wave taking at most ceil(items / waves) rays at a time, and scans
			// cooperatively throughout (profiles/r03/sparse_launch.txt).
			if (sparse_launch)
			{
				constexpr uint64_t launch_waves = 256ull * 4ull * 5ull;
				const uint64_t items = static_cast<uint64_t>(width) * local_rows * (q.halves ? (samples_per_pixel + q.item_samples - 1u) / q.item_samples : q.chunks);
				const uint64_t per_wave = (items + launch_waves - 1u) / launch_waves;
				if (per_wave <= 32u)
				{
					q.lane_cap = static_cast<uint32_t>(std::max<uint64_t>(per_wave, 1u));
					q.block_items = std::min(q.block_items, q.lane_cap);
					q.sparse_rays = std::max(q.sparse_rays, q.lane_cap);
				}
			}
		}
		else
		{
			// one tile per wave.  A wave lives as long as its longest lane and the launch ends with about one wave lifetime
			// of tail, so waves should be short — but with fewer than two items per lane the lanes of a wave end at very
			// different times.  Measured on the headline frame and on its 1/2, 1/4, 1/8 shares at 256, 64 and 16 spp
			// (profiles/r01/queue_shape_sweep.txt): 128 items per wave, and 64 when that would give fewer than 6 x 8192
			// waves (8192 = what the device holds at a time), win or tie every case.
			pixels_log2 = 7; // 128 pixels = 16 x 8
			while (pixels_log2 > 2 && (q.chunks << pixels_log2) > 128u)
				pixels_log2--;
			const uint64_t pixels = static_cast<uint64_t>(width) * local_rows;
			if (pixels_log2 > 2 && (pixels >> pixels_log2) < 49152u)
				pixels_log2--;
		}
		// Half-chunks (render_queue<.., HALF>): a launch that has only a few chunks per lane of the device ends unevenly —
		// a rank's 1/8 share of a 64-spp frame holds two per lane and took 0.21 ms for 0.09 ms of work; with 8-sample items
		// 0.13-0.14 (profiles/r03/chunk_probe.txt: 1/4 share -11 %, nothing from eight chunks per lane upwards, where the
		// parking would only cost).  64 half-chunks per wave, one per lane; tiles of at least four pixels.
		// (Not for pixels of ONE chunk, forced aside: their tiles would hold half as many pixels and the wave's fold — a
		// division and three square roots per pixel — runs on half its lanes: 1080p x 16 spp 0.345 against 0.323 ms.  Between
		// four and seven chunks per lane the gain fades: 800 x 600 x 64 spp -16 %, 1280 x 720 x 64 spp +16 %;
		// profiles/r03/half_threshold.txt.)
		if (half_chunks && !big_scene && samples_per_pixel > sample_chunk / 2u && q.chunks <= 16u)
		{
			constexpr uint64_t resident_lanes = 256ull * 4ull * 8ull * 64ull; // an MI355X at 8 waves per SIMD
			if (half_chunks == 2 || (q.chunks >= 2u && static_cast<uint64_t>(width) * local_rows * q.chunks < 5ull * resident_lanes))
			{
				q.halves = 1u;
				pixels_log2 = 2u;
				while (pixels_log2 < 7u && ((2u * q.chunks) << (pixels_log2 + 1u)) <= 64u)
					pixels_log2++;
			}
		}
		// frames of headline size and beyond at 256 spp: 16 pixels (256 items) per wave beat 8 — half as many waves to start
		// and to fold (HBM: 2.62 against 2.63 ms at 1080p, 10.4 against 10.6 at 4K; profiles/r03/tile_shapes.txt) — while a
		// half frame still prefers 8 (1.39 against 1.34)
		if (!big_scene && !q.halves && pixels_log2 == 3u && (q.chunks << 4u) <= 256u && ((static_cast<uint64_t>(width) * local_rows) >> 4u) >= 98304u)
			pixels_log2 = 4u;
		q.pixels_log2 = pixels_log2;
		q.tile_w_log2 = (pixels_log2 + 1u) / 2u; // 16x8, 8x8, 8x4, 4x4, 4x2, 2x2, 2x1, 1x1
		if (host_frame && !big_scene && q.halves)
			q.tile_w_log2 = std::min(pixels_log2, 4u); // (rows as wide as the tile allows: see below)
		else if (host_frame && !big_scene)
		{
			// The finished pixels of a tile leave the wave as one store per tile, a row fragment of tile_w pixels per tile
			// row; into page-locked host memory every fragment is a PCIe write.  Fragments of 8 and 16 bytes (2 x 2, 4 x 4,
			// 4 x 2 tiles) cost nothing in HBM and a lot over PCIe as soon as there are many of them per microsecond — a 1/8
			// share of the headline frame took 0.60 ms as 2 x 2 tiles against 0.35 ms into HBM, 0.37 ms as 4 x 1; config 2's
			// whole frame 1.36 ms into memory of the other socket as 8 x 4, 0.86 ms as 16 x 2 — and so does memory on the far
			// socket (profiles/r03/tile_shapes.txt).  So: rows as wide as the tile allows, up to 64 bytes.  One exception,
			// where the launch has waves to spare: 256-spp frames of headline size take 16 pixels as 8 x 2 instead of 8 as
			// 8 x 1 (half as many store instructions: as fast as the frame left in HBM whichever socket the memory is on).
			const uint64_t pixels = static_cast<uint64_t>(width) * local_rows;
			if (pixels_log2 == 3u && (q.chunks << 4u) <= 256u && (pixels >> 4u) >= 49152u)
				q.pixels_log2 = pixels_log2 = 4u;
			// (16 pixels at 256 spp: 8 x 2 for the 1..4-sphere kernels — basic.toml 2.639 against 2.664 ms as 16 x 1 — and 16 x 1
			// for the 5..8-sphere and the resident ones — dielectric.toml 3.011 against 3.040 as 8 x 2; tile_sweep_drop_in.txt)
			q.tile_w_log2 = (pixels_log2 == 4u && q.chunks == 16u && primitives < 5u) ? 3u : std::min(pixels_log2, 4u);
		}
#ifdef RT_HIP_QUEUE_KNOBS
		// experiment builds only (tools/gpu_tile_shapes.py): tile size and width from the environment, per launch
		if (!big_scene)
		{
			if (const char* knob = std::getenv("RT_HIP_TILE_LOG2"))
				q.pixels_log2 = pixels_log2 = static_cast<uint32_t>(std::atoi(knob));
			q.tile_w_log2 = (pixels_log2 + 1u) / 2u;
			if (const char* knob = std::getenv("RT_HIP_TILE_W_LOG2"))
				q.tile_w_log2 = std::min<uint32_t>(static_cast<uint32_t>(std::atoi(knob)), pixels_log2);
		}
#endif
		cut_tiles(q, width, local_rows);
		return q;
	}

	void rolling_buffer_bytes(const queue_params& queue, uint32_t samples_per_pixel, uint32_t width, uint32_t local_rows, bool big_scene, size_t& item_sums_bytes, size_t& pixel_done_bytes)
	{
		item_sums_bytes = pixel_done_bytes = 0;
		if (!big_scene || (queue.chunks <= 1u && !queue.halves)) // one chunk per pixel: the lane that traced it writes the pixel
			return;
		const size_t pixels = static_cast<size_t>(width) * local_rows;
		item_sums_bytes = queue.halves ? pixels * samples_per_pixel * 16u : pixels * queue.chunks * 16u;
		pixel_done_bytes = pixels * sizeof(uint32_t);
	}

	launch_plan plan_launch(const launch_request& request)
	{
		launch_plan plan{};
		const uint64_t pixels = static_cast<uint64_t>(request.width) * request.local_rows;
		uint32_t kernel = choose_kernel(request.n_spheres, request.n_planes, request.planes_tame, request.flags, request.samples_per_pixel, request.camera != camera_form::other, pixels);
		// A pass of a progressive frame: only the tile-per-wave whole-chunk kernels have a pass build (kernels.hip, render_queue: PASS).  A scene
		// of the streamed kernel's size goes through the sphere hierarchy, a scene of the scalar-register kernel's takes the resident one (as
		// under RT_HIP_FLAG_FORCE_RESIDENT); the queue is cut for the PASS's samples, in whole chunks.  (The API admits no FORCE_ flag here.)
		const bool pass = request.pass_samples != 0u;
		if (pass)
			kernel = (kernel == RT_HIP_KERNEL_BVH || kernel == RT_HIP_KERNEL_STREAMED) ? RT_HIP_KERNEL_BVH : RT_HIP_KERNEL_RESIDENT;
		// Traced boxes (RT_HIP_FLAG_TRACE_BOXES and at least one box) are planned like a pass: the box builds are builds of the two
		// tile-per-wave kernels, in whole chunks.  The scalar-register builds live at their register budget and get no box code: their scenes
		// take the resident kernel.  Without the flag, or without a box, nothing below differs from the frame as it always was.
		const bool boxes = (request.flags & RT_HIP_FLAG_TRACE_BOXES) && request.n_boxes != 0u;
		if (boxes)
			kernel = (kernel == RT_HIP_KERNEL_BVH || kernel == RT_HIP_KERNEL_STREAMED) ? RT_HIP_KERNEL_BVH : RT_HIP_KERNEL_RESIDENT;
		// RT_HIP_FLAG_BOX_BVH: the boxes through their own hierarchy, which walks the hierarchy kernel's per-lane stacks — that kernel
		// whatever the sphere count (its sphere tree may be empty)
		const bool box_tree = boxes && (request.flags & RT_HIP_FLAG_BOX_BVH);
		if (box_tree)
			kernel = RT_HIP_KERNEL_BVH;
		// Lights (RT_HIP_FLAG_EMISSION and at least one light in the context's table) are planned like traced boxes: the light builds are
		// builds of the two tile-per-wave kernels, in whole chunks; scenes of the scalar-register kernels' size take the resident one, scenes
		// of the streamed kernel's the hierarchy.  (The API refuses the flag with passes, boxes and the FORCE_ flags.)  Without the flag, or
		// without a light, nothing below differs from the frame as it always was.
		const bool lights = (request.flags & RT_HIP_FLAG_EMISSION) && request.n_lights != 0u && !pass && !boxes;
		if (lights)
			kernel = (kernel == RT_HIP_KERNEL_BVH || kernel == RT_HIP_KERNEL_STREAMED) ? RT_HIP_KERNEL_BVH : RT_HIP_KERNEL_RESIDENT;
		// A lens (RT_HIP_FLAG_THIN_LENS and an aperture radius above 0 in the context's lens) is planned like lights: the lens builds are builds
		// of the two tile-per-wave kernels, in whole chunks; scenes of the scalar-register kernels' size take the resident one, scenes of the
		// streamed kernel's the hierarchy.  (The API refuses the flag with passes, boxes, lights and the FORCE_ flags.)  Without the flag, or
		// with a radius of 0, nothing below differs from the frame as it always was.
		const bool lens = (request.flags & RT_HIP_FLAG_THIN_LENS) && request.lens_aperture > 0.0f && !pass && !boxes && !lights;
		if (lens)
			kernel = (kernel == RT_HIP_KERNEL_BVH || kernel == RT_HIP_KERNEL_STREAMED) ? RT_HIP_KERNEL_BVH : RT_HIP_KERNEL_RESIDENT;
		plan.variant = pixels ? kernel : static_cast<uint32_t>(RT_HIP_KERNEL_NONE);
		const bool big_scene = plan.big_scene = kernel == RT_HIP_KERNEL_TILED || kernel == RT_HIP_KERNEL_STREAMED;
		queue_params queue = choose_queue(pass ? request.pass_samples : request.samples_per_pixel, request.width, request.local_rows, big_scene, request.host_frame, (pass || boxes || lights || lens) ? 0 : half_chunk_choice(request.flags),
															 request.n_spheres + request.n_planes, kernel == RT_HIP_KERNEL_STREAMED && request.n_spheres >= sparse_launch_min_spheres);
		// An adaptive pass: the wave's stop mask is one ballot of its tile's state words — a tile of at most 64 pixels.  choose_queue cuts
		// 128-pixel tiles for one-chunk passes of frames beyond 6M pixels only; those are halved here (the short side first, as it would).
		const bool adaptive = pass && request.adaptive;
		if (adaptive && (1u << queue.pixels_log2) > adaptive_max_tile_pixels)
		{
			queue.pixels_log2 = 6u;
			queue.tile_w_log2 = std::min(queue.tile_w_log2, 4u); // (64 pixels: 8 x 8, or 16 x 4 for a page-locked frame)
			if (!request.host_frame)
				queue.tile_w_log2 = 3u;
			cut_tiles(queue, request.width, request.local_rows);
		}
		plan.queue = queue;
		plan.build.pass = pass;
		plan.build.adaptive = adaptive;
		plan.build.boxes = boxes;
		plan.build.box_tree = box_tree;
		plan.build.lights = lights;
		plan.build.direct = lights && request.n_sampled_lights != 0u; // (the caller counts sampled lights under RT_HIP_FLAG_DIRECT_LIGHT only)
		plan.build.lens = lens;
		plan.first_chunk = pass ? request.pass_first_sample / sample_chunk : 0u;

		// small scenes: one wave per tile, four tiles side by side per workgroup.  Big scenes: a persistent launch — what
		// the device keeps resident, and no more lanes than items
		plan.total_items = pixels * ((big_scene && queue.halves) ? (request.samples_per_pixel + queue.item_samples - 1u) / queue.item_samples : queue.chunks);
		const uint64_t items_per_workgroup = big_scene ? static_cast<uint64_t>(block_threads / 64u) * queue.lane_cap : block_threads; // (a sparse launch: lane_cap rays per wave)
		plan.grid_x = big_scene ? static_cast<uint32_t>(std::min<uint64_t>(0x7FFFFFFFull, (plan.total_items + items_per_workgroup - 1u) / items_per_workgroup)) // capped to the resident count at launch
								: (queue.tiles_x + 3u) / 4u;
		plan.grid_y = big_scene ? 1u : queue.tiles_y;
		// small scenes: a pixel's chunk sums (one per 16 samples) are parked in LDS until the pixel is complete
		plan.slot_bytes = big_scene ? 0u : static_cast<size_t>(block_threads / 64u) * tile_slot_bytes(queue);
		// big scenes: they meet in HBM, 16 bytes per chunk (or per sample) of this rank's rows
		rolling_buffer_bytes(queue, request.samples_per_pixel, request.width, request.local_rows, big_scene, plan.item_sums_bytes, plan.pixel_done_bytes);

		constexpr size_t float4_bytes = 16;
		const bool pinhole = request.camera == camera_form::pinhole;
		kernel_build& build = plan.build;
		build.sm_table = (request.flags & RT_HIP_FLAG_SM_MATERIALS) != 0;
		build.sub_chunk_items = queue.halves != 0; // (never with the sm table, which keeps whole chunks: half_chunk_choice)
		switch (kernel)
		{
			case RT_HIP_KERNEL_SMALL: // (choose_kernel admits n_spheres + n_planes <= 8 only)
				build.scan = static_cast<int>(request.n_spheres);
				build.planes = static_cast<int>(request.n_planes);
				build.general_camera = !pinhole;
				plan.table_bytes = small_table_float4s * float4_bytes;
				break;
			case RT_HIP_KERNEL_BVH:
				build.scan = scan_bvh;
				plan.table_bytes = bvh_stack_float4s * float4_bytes;
				break;
			case RT_HIP_KERNEL_RESIDENT:
				build.scan = scan_resident;
				build.planes = request.n_spheres >= resident_scalar_scan_from ? 1 : 0; // (the scalar-load scan: one build for every camera form)
				build.general_camera = build.planes == 0 && !pinhole;
				plan.table_bytes = static_cast<size_t>((request.n_spheres < resident_scalar_scan_from ? request.n_spheres : 0u) + request.n_planes) * float4_bytes;
				break;
			case RT_HIP_KERNEL_STREAMED:
			{
				// A frame that fills the device — not a thin launch, and at least 4M samples — takes the build without the cooperative scan of
				// sparse waves: only its last waves run sparse, and the registers that scan costs every other trip are worth 9 % (config 5).
				const bool dense = queue.lane_cap == 64u && pixels * request.samples_per_pixel >= (1ull << 22);
				build.scan = dense ? scan_streamed_dense : scan_streamed;
				break;
			}
			default:
				build.scan = scan_tiled;
				plan.table_bytes = tile_primitives * float4_bytes;
				break;
		}
		if (box_tree)
		{
			// nothing is staged: the stacks alone, and no cap on the count (the tree's own is the builder's to refuse)
			if (plan.table_bytes + plan.slot_bytes > workgroup_lds_bytes)
				std::snprintf(plan.refusal, sizeof(plan.refusal), "RT_HIP_FLAG_BOX_BVH: %zu bytes of stacks and %zu of chunk sums do not fit a workgroup's %zu bytes of LDS", plan.table_bytes, plan.slot_bytes, workgroup_lds_bytes);
		}
		else if (boxes)
		{
			// the boxes' corners behind the scan's own table: the planes (and LDS-scanned spheres) of the resident kernel, the hierarchy kernel's stacks
			plan.table_bytes += static_cast<size_t>(request.n_boxes) * 2u * float4_bytes;
			if (request.n_boxes > box_max_count)
				std::snprintf(plan.refusal, sizeof(plan.refusal), "RT_HIP_FLAG_TRACE_BOXES: %u boxes: at most %u are traced (a linear scan from LDS; there is no hierarchy over boxes)", request.n_boxes, box_max_count);
			else if (plan.table_bytes + plan.slot_bytes > workgroup_lds_bytes)
				std::snprintf(plan.refusal, sizeof(plan.refusal), "RT_HIP_FLAG_TRACE_BOXES: %zu bytes of tables and %zu of chunk sums do not fit a workgroup's %zu bytes of LDS", plan.table_bytes, plan.slot_bytes, workgroup_lds_bytes);
			else if (plan.slot_bytes > max_slot_bytes) // (the resident kernel's box builds, whose tables leave room: the one-shot limit, said by the plan —
													   // max_slot_bytes of four tiles of four pixels, 12 bytes per chunk and pixel)
				std::snprintf(plan.refusal, sizeof(plan.refusal), "RT_HIP_FLAG_TRACE_BOXES: %u samples per pixel are more than the box builds hold chunk sums for (%u)", request.samples_per_pixel,
							  static_cast<uint32_t>(max_slot_bytes / (block_threads / 64u * 4u * 3u * sizeof(float)) * sample_chunk));
		}
		plan.lds_bytes = plan.table_bytes + plan.slot_bytes;
		// No plan is launched that the device cannot hold.  (Slots beyond max_slot_bytes are refused by the sample count: render.hip.)  How many
		// samples do fit: at such a count a tile holds four pixels whatever the count (choose_queue: from 33 chunks on), so the slots grow by
		// the same bytes per chunk all the way down to the limit.
		const size_t lds_limit = request.lds_limit ? request.lds_limit : workgroup_lds_bytes;
		if (!plan.refusal[0] && !big_scene && plan.slot_bytes <= max_slot_bytes && plan.lds_bytes > lds_limit)
		{
			const size_t per_chunk = plan.slot_bytes / queue.chunks;
			const size_t fit = plan.table_bytes < lds_limit ? (lds_limit - plan.table_bytes) / per_chunk * sample_chunk : 0u;
			std::snprintf(plan.refusal, sizeof(plan.refusal), "%s%u samples%s need%s %zu bytes of LDS (%zu of tables, %zu of chunk sums) and a workgroup of this device has %zu: at most %zu samples fit", pass ? "a pass of " : "",
						  pass ? request.pass_samples : request.samples_per_pixel, pass ? "" : " per pixel", pass ? "s" : "", plan.lds_bytes, plan.table_bytes, plan.slot_bytes, lds_limit, fit);
		}

		// what the context remembers of a persistent kernel (launch_cache): one entry per kernel, table and item size
		plan.persistent_slot = -1;
		if (scan_is_persistent(build.scan))
		{
			const unsigned kernel_index = build.scan == scan_tiled ? 0u : (build.scan == scan_streamed ? 1u : 2u);
			plan.persistent_slot = static_cast<int>((build.sub_chunk_items ? 9u : 0u) + 3u * kernel_index + (request.fast_arithmetic ? 2u : (build.sm_table ? 1u : 0u)));
			plan.per_cu_cap = build.scan == scan_streamed_dense ? RT_HIP_WAVES_DENSE : RT_HIP_PERSISTENT_WAVES_CAP;
		}
		return plan;
	}
}
