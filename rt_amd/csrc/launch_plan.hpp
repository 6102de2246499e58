// rt_amd/csrc/launch_plan.hpp — every host decision of one render launch, made ONCE (plan_launch): which kernel, which build of
// it, the shape of its work, its grid and LDS, the HBM buffers it needs.  render.hip plans a launch, prepares what the plan asks
// for and hands the same plan to launch_render (kernels.hip), which only picks the instantiation and launches it.
// Host-only integer policy with the measurements that justify it: plain C++17, no HIP header, built with the host compiler into
// librt_hip.so and, on the CPU, into tests/native/launch_plan_dump (tests/test_launch_plan.py pins every decision).
#pragma once

#include <stdint.h>
#include <stddef.h>
#include "../../include/rt_hip.h" // (the render flags and RT_HIP_KERNEL_*)

// waves per SIMD the streamed kernel of frames that fill the device is compiled for (scan_streamed_dense: no cooperative scan of sparse
// waves, whose four 16-byte loads in flight per lane set the register count of the other build): 80 registers hold its loop, half-chunk
// items included — config 5 5.47 s at 5 waves WITH the cooperative scan, 5.09 without, 4.99 at 6 waves, 5.05 at 7
// (profiles/r05/streamed_occupancy_ab.txt)
#ifndef RT_HIP_WAVES_DENSE
#define RT_HIP_WAVES_DENSE 6
#endif
#ifndef RT_HIP_PERSISTENT_WAVES_CAP
#define RT_HIP_PERSISTENT_WAVES_CAP 5 // workgroups per CU of the persistent (big-scene) launches: see launch_render
#endif

namespace rt_hip
{
	constexpr uint32_t block_threads = 256; // a workgroup of the render kernels: 4 waves

	// the whole scene of the `small` kernel is passed by value as a kernel argument (-> SGPRs): small_scene, kernels.hpp
	constexpr uint32_t scalar_max_spheres = 8; // scenes of up to this many primitives (spheres + planes) run with the scene in SGPRs
	constexpr uint32_t scalar_max_planes = 3;  // ... of which at most this many planes (and at least one sphere)
	constexpr uint32_t small_table_float4s = 2u * scalar_max_spheres; // LDS tables of the scalar-register kernels: geometry, shading

	// pixel sums are taken in chunks of this many consecutive samples (arithmetic contract; see oracle/cpu_ref.cpp)
#ifdef RT_HIP_SAMPLE_CHUNK // (timing experiments only: frames of such a build are not the contract's)
	constexpr uint32_t sample_chunk = RT_HIP_SAMPLE_CHUNK;
#else
	constexpr uint32_t sample_chunk = 16;
#endif

	// Work distribution.  The unit of work is one ITEM = one chunk of 16 consecutive samples of one pixel (K = chunks per
	// pixel).  Small scenes: the frame is cut into pixel tiles of P = 2^pixels_log2 pixels, one tile (P x K items) per wave,
	// launched as a grid of tiles.  Big scenes (tiled / streamed kernels): a persistent launch whose waves draw single
	// items, in blocks of `block_items`, from one launch-wide sequence (device_counters::next_item), pixel-major, bottom
	// row first; a pixel's chunk sums meet in HBM (rolling_buffers).
	struct queue_params
	{
		uint32_t chunks;		   // K = ceil(spp / sample_chunk)
		uint32_t pixels_log2;	   // P (small scenes)
		uint32_t tile_w_log2;	   // a tile is 2^tile_w_log2 columns wide
		uint32_t tiles_x, tiles_y; // tiles across / down this rank's rows
		uint32_t block_items;	   // big scenes: items a wave draws from the launch-wide sequence at a time
		uint32_t lane_cap;		   // big scenes: rays a wave holds at most (64 = all lanes; less in sparse launches of the streamed kernel)
		uint32_t sparse_rays;	   // streamed kernel: a wave holding at most this many rays scans cooperatively
		uint32_t halves;		   // short launches: 1 = the work items are smaller than a chunk (render_queue<.., HALF>): small scenes
								   // half chunks; big scenes item_samples consecutive samples, every sample's value parked
		uint32_t item_samples;	   // big scenes with halves: samples per work item (8, 4, 2 or 1)
	};
	// LDS floats per chunk of a tile: its sum — or, with half-chunks, the first half's partial sum and the second half's 8 x 3 sample values
	constexpr uint32_t half_chunk_slot_floats = 3u + 3u * (sample_chunk / 2u);
	inline size_t tile_slot_bytes(const queue_params& q) // of ONE wave's tile
	{
		return static_cast<size_t>(q.chunks << q.pixels_log2) * (q.halves ? half_chunk_slot_floats : 3u) * sizeof(float);
	}
	// `host_frame`: the packed pixels go to page-locked HOST memory (every row fragment of a tile is a PCIe write)
	// `half_chunks`: 0 = whole chunks (the sm table's kernels have no half-chunk build; RT_HIP_FLAG_FORCE_WHOLE_CHUNKS),
	// 1 = by the size of the launch, 2 = half chunks wherever the samples allow (RT_HIP_FLAG_FORCE_HALF_CHUNKS)
	queue_params choose_queue(uint32_t samples_per_pixel, uint32_t width, uint32_t local_rows, bool big_scene, bool host_frame, int half_chunks, uint32_t primitives, bool sparse_launch);
	constexpr uint32_t sparse_wave_rays = 8;			 // (streamed kernel) a wave holding at most this many rays scans together
	constexpr uint32_t sparse_launch_min_spheres = 1024; // the streamed kernel's cooperative scan (a wave with a handful of rays) exists from here
	inline int half_chunk_choice(uint32_t flags)
	{
		if (flags & (RT_HIP_FLAG_SM_MATERIALS | RT_HIP_FLAG_FORCE_WHOLE_CHUNKS))
			return 0;
		return (flags & RT_HIP_FLAG_FORCE_HALF_CHUNKS) ? 2 : 1;
	}

	// bytes of the two buffers the big-scene kernels exchange chunk sums through (rolling_buffers, kernels.hpp) for a launch
	// (0, 0 for the small-scene kernels)
	void rolling_buffer_bytes(const queue_params& queue, uint32_t samples_per_pixel, uint32_t width, uint32_t local_rows, bool big_scene, size_t& item_sums_bytes, size_t& pixel_done_bytes);

#ifndef RT_HIP_RESIDENT_SCALAR_FROM
#define RT_HIP_RESIDENT_SCALAR_FROM 40
#endif
	constexpr uint32_t resident_scalar_scan_from = RT_HIP_RESIDENT_SCALAR_FROM; // spheres from which the resident kernel scans through the scalar cache (kernels.hip)
	constexpr uint32_t resident_max_primitives = 1024; // what the resident kernel keeps in LDS at most: the planes, and the spheres of a scene below resident_scalar_scan_from
	// The launch code prefers the resident kernel (a pixel tile per wave) up to this many primitives, the streamed kernel's rolling
	// items beyond.  From resident_scalar_scan_from spheres on the resident kernel reads the sphere table in memory, as the streamed
	// kernel does, and its LDS holds planes only — so its capacity is no limit to the spheres; what ends its lead is that a tile's
	// lanes run dry one by one while a trip costs the wave a whole scan.  Against the streamed kernel's build for dense frames
	// (1080p x 64 spp, kernel ms): 400 spheres 16.8 against 18.4, 700: 29.7 against 31.0, 1 000: 42.9 against 44.9, 1 100: 47.8 against
	// 48.4, 1 500: 66.5 against 65.8, 2 000: 90.3 against 87.9, 3 000: 141.8 against 130.7 (profiles/r05/resident_vs_dense_streamed.txt;
	// against the streamed kernel as it was before that build the lead lasted to 4 000 spheres: resident_beyond_1024_ab.txt).
	constexpr uint32_t streamed_from_primitives = 1300;
	constexpr uint32_t bvh_stack_float4s = 24u * 256u / 4u; // the BVH kernel's LDS traversal stacks: bvh_max_depth words per thread (bvh.hpp, kernels.hip)
	constexpr uint32_t tile_primitives = 1024;		   // primitives per LDS tile in the tiled kernel
	// RT_HIP_FLAG_TRACE_BOXES: the box builds scan the boxes linearly from LDS, two float4s each (the corners), staged behind the scan's own
	// table — 8 KiB at the most.  (RT_HIP_FLAG_BOX_BVH's frames reach the boxes through a hierarchy instead and know no such cap.)
	constexpr uint32_t box_max_count = 256;
	constexpr size_t workgroup_lds_bytes = 64u * 1024u; // what one workgroup may ask for where the device has not been asked (launch_request::lds_limit), and what the box builds are planned within
	constexpr size_t max_slot_bytes = 48u * 1024u;		// chunk-sum slots of a workgroup's four tiles at the most: 4096 samples (render.hip refuses more by the sample count)

	// which kernel a launch takes (RT_HIP_KERNEL_*)
	uint32_t choose_kernel(uint32_t n_spheres, uint32_t n_planes, bool planes_tame /* device_scene::planes_tame */, uint32_t flags, uint32_t samples_per_pixel,
						   bool perspective /* the frame's camera is a pinhole or a plain eye-form one: frame_params::pinhole or eye_form == 2 */, uint64_t pixels /* of this rank's rows */);

	// The scan a build of render_queue<NS, ..> is compiled for, as its first template argument says it: NS > 0 is the `small`
	// kernel with NS spheres in scalar registers; the other kernels have these codes (kernels.hip, render_queue).
	enum : int
	{
		scan_resident = 0,		  // all primitives in LDS — or, NP == 1, the planes in LDS and the spheres through scalar loads
		scan_tiled = -1,		  // rolling items; the primitives stream through one LDS tile per workgroup
		scan_streamed = -2,		  // rolling items; wave-uniform scalar loads, sparse waves scan cooperatively
		scan_streamed_dense = -3, // ... without the cooperative scan: frames that fill the device
		scan_bvh = -4,			  // RT_HIP_FLAG_BVH: a pixel tile per wave, spheres through the hierarchy
		// the PASS builds of the two tile-per-wave scans (kernel_build::pass; progressive frames): the same scans, a fold that continues
		scan_resident_pass = -5,
		scan_bvh_pass = -6,
		// the BOX builds of the same two scans (kernel_build::boxes; RT_HIP_FLAG_TRACE_BOXES): the scene's boxes staged into LDS behind
		// the scan's own table and scanned after spheres and planes
		scan_resident_boxes = -7,
		scan_bvh_boxes = -8,
		// RT_HIP_FLAG_BOX_BVH (kernel_build::box_tree): the hierarchy kernel with the boxes reached through a hierarchy of their own
		// (box_bvh_scan.hpp) on the same per-lane stacks — nothing staged into LDS, no cap of box_max_count
		scan_bvh_boxtree = -9,
		// the ADAPTIVE builds of the two pass builds (kernel_build::adaptive): a pass that reads the pixels' state words,
		// traces and folds the active pixels only, stores the pass's own fold next to the running sum and finishes no pixel
		scan_resident_adapt = -10,
		scan_bvh_adapt = -11,
		// the LIGHT builds of the same two scans (kernel_build::lights; RT_HIP_FLAG_EMISSION with at least one light): a hit
		// whose scatter row says scatter_emit ends the sample with throughput * the row's shading.rgb — the same scan, whole chunks only
		scan_resident_lights = -12,
		scan_bvh_lights = -13,
		// the DIRECT builds of the light builds (kernel_build::direct; RT_HIP_FLAG_DIRECT_LIGHT with at least one sampled light):
		// a lambert vertex aims a shadow segment at a sampled sphere light before it scatters — light builds in everything else
		scan_resident_direct = -14,
		scan_bvh_direct = -15,
		// the LENS builds of the same two scans (kernel_build::lens; RT_HIP_FLAG_THIN_LENS with an aperture): the restart draws
		// one more generator step and bends the primary ray it has just made through a point of the lens — the same scan, whole chunks only
		scan_resident_lens = -16,
		scan_bvh_lens = -17
	};
	constexpr bool scan_has_lens(int code) { return code == scan_resident_lens || code == scan_bvh_lens; }
	constexpr bool scan_has_direct(int code) { return code == scan_resident_direct || code == scan_bvh_direct; }
	constexpr bool scan_has_lights(int code) { return code == scan_resident_lights || code == scan_bvh_lights || scan_has_direct(code); }
	constexpr bool scan_is_adaptive(int code) { return code == scan_resident_adapt || code == scan_bvh_adapt; }
	constexpr bool scan_is_pass(int code) { return code == scan_resident_pass || code == scan_bvh_pass || scan_is_adaptive(code); }
	constexpr bool scan_has_boxes(int code) { return code == scan_resident_boxes || code == scan_bvh_boxes || code == scan_bvh_boxtree; }
	constexpr bool scan_has_box_tree(int code) { return code == scan_bvh_boxtree; }
	constexpr int scan_of(int code) // the scan a build's code stands for
	{
		return (code == scan_resident_pass || code == scan_resident_boxes || code == scan_resident_adapt || code == scan_resident_lights || code == scan_resident_direct || code == scan_resident_lens)
				   ? static_cast<int>(scan_resident)
				   : ((code == scan_bvh_pass || code == scan_bvh_boxes || code == scan_bvh_boxtree || code == scan_bvh_adapt || code == scan_bvh_lights || code == scan_bvh_direct || code == scan_bvh_lens) ? static_cast<int>(scan_bvh) : code);
	}
	// the rolling kernels are launched persistent: as many workgroups as the device keeps resident (launch_cache, kernels.hpp)
	constexpr bool scan_is_persistent(int scan) { return scan == scan_tiled || scan == scan_streamed || scan == scan_streamed_dense; }
	constexpr unsigned persistent_cache_slots = 18; // { tiled, streamed, streamed for dense frames } x { mg, sm scatter table, fast arithmetic } x { whole chunks, sub-chunk items }

	enum class camera_form : uint32_t
	{
		pinhole,   // frame_params::pinhole
		plain_eye, // frame_params::eye_form == 2
		other	   // an eye form that needs its guards, or the homogeneous form
	};

	// what a launch is planned from
	struct launch_request
	{
		uint32_t n_spheres, n_planes;
		bool planes_tame; // device_scene::planes_tame
		uint32_t width, local_rows, samples_per_pixel; // this rank's rows of the frame
		camera_form camera;
		uint32_t flags;		  // RT_HIP_FLAG_*
		bool host_frame;	  // the packed pixels go to page-locked host memory (choose_queue)
		bool fast_arithmetic; // RT_HIP_FLAG_FAST's build of the kernels (launch_render_fast)
		// One PASS of a progressive frame (pass_samples != 0): samples [pass_first_sample, pass_first_sample + pass_samples) of every pixel,
		// folded onto the pixels' running sums.  pass_first_sample is a multiple of sample_chunk; samples_per_pixel stays the frame's.
		// Both 0: a frame in one launch, planned as it always was.
		uint32_t pass_first_sample = 0, pass_samples = 0;
		// RT_HIP_FLAG_TRACE_BOXES: the resident scene's boxes (device_scene::n_boxes).  Without the flag, or with none, a frame is planned
		// as it always was, field for field.  With RT_HIP_FLAG_BOX_BVH too (and at least one box) the frame is planned onto the hierarchy
		// kernel's scan_bvh_boxtree build whatever the sphere count, with the stacks as its only table.
		uint32_t n_boxes = 0;
		// An ADAPTIVE pass (set by the adaptive entry points only, with pass_samples != 0): the pass's adaptive build, whose
		// waves ballot their tile's state words into ONE 64-bit stop mask — so a tile holds at most adaptive_max_tile_pixels pixels.
		bool adaptive = false;
		// RT_HIP_FLAG_EMISSION: how many materials of the context's emission table are lights.  Without the flag, or with none (the
		// default: "no lights"), a frame is planned as it always was, field for field; with at least one it is planned like a box frame,
		// onto the light builds of the two tile-per-wave kernels.
		uint32_t n_lights = 0;
		// RT_HIP_FLAG_DIRECT_LIGHT: how many SAMPLED lights the resident scene has under that table.  With none the frame is
		// planned as the RT_HIP_FLAG_EMISSION frame, field for field — the plan looks at this count, not at the flag.
		uint32_t n_sampled_lights = 0;
		// RT_HIP_FLAG_THIN_LENS: the aperture radius of the context's lens.  Without the flag, or with a radius of 0, a frame is
		// planned as it always was, field for field — the plan looks at the radius, not at the flag alone; with an aperture it is planned
		// like a light frame, onto the lens builds of the two tile-per-wave kernels.
		float lens_aperture = 0.0f;
	// LDS bytes a workgroup of the device may ask for (the context reads it off the device's properties); 0: workgroup_lds_bytes.  A plan
	// of a tile-per-wave kernel whose tables and chunk sums need more is refused, whatever the build: only the hierarchy kernel's — 24 KiB
	// of stacks in front of the slots — can, from 3409 samples (a frame's, or a pass's) at a limit of 64 KiB.
	size_t lds_limit = 0;
	};
	constexpr uint32_t adaptive_max_tile_pixels = 64;

	// the instantiation render_queue<scan, sm_table, sub_chunk_items, planes, general_camera>
	struct kernel_build
	{
		int scan;			  // NS: the spheres of a scalar-register kernel, or scan_*
		int planes;			  // NP: the planes of a scalar-register kernel; scan_resident: 1 = the scalar-load scan
		bool general_camera;  // GC: the frame is not a pinhole's (scalar-register kernels and the resident LDS scan)
		bool sub_chunk_items; // HALF
		bool sm_table;		  // SM: RT_HIP_FLAG_SM_MATERIALS
		bool pass;			  // one pass of a progressive frame: the scan's PASS build (scan_resident_pass / scan_bvh_pass; `scan` stays the scan proper)
		bool boxes;			  // RT_HIP_FLAG_TRACE_BOXES with at least one box: the scan's BOX build (scan_resident_boxes / scan_bvh_boxes)
		bool box_tree;		  // ... and RT_HIP_FLAG_BOX_BVH: the hierarchy kernel's scan_bvh_boxtree build (`boxes` is set too)
		bool adaptive;		  // an adaptive pass: the scan's ADAPT build (scan_resident_adapt / scan_bvh_adapt; implies `pass`)
		bool lights;		  // RT_HIP_FLAG_EMISSION with at least one light: the scan's LIGHT build (scan_resident_lights / scan_bvh_lights)
		bool direct;		  // ... and at least one sampled light (RT_HIP_FLAG_DIRECT_LIGHT): its DIRECT build (scan_resident_direct / scan_bvh_direct; `lights` is set too)
		bool lens;			  // RT_HIP_FLAG_THIN_LENS with an aperture: the scan's LENS build (scan_resident_lens / scan_bvh_lens)
	};

	struct launch_plan
	{
		uint32_t variant; // RT_HIP_KERNEL_*; RT_HIP_KERNEL_NONE for a frame without pixels: nothing is launched (the other fields
						  // are still those of the kernel the scene would take)
		bool big_scene;	  // a rolling kernel (tiled / streamed): items drawn from device_counters::next_item, which must start at 0
		queue_params queue;
		kernel_build build;
		uint32_t grid_x, grid_y; // workgroups; a persistent launch is capped to what the device keeps resident at launch (launch_render)
		size_t table_bytes;		 // LDS: the primitive tables / the tiled kernel's tile / the BVH kernel's stacks ...
		size_t slot_bytes;		 // ... and the chunk-sum slots of the workgroup's four tiles (small scenes)
		size_t lds_bytes;		 // = table_bytes + slot_bytes
		uint64_t total_items;
		size_t item_sums_bytes, pixel_done_bytes; // rolling_buffer_bytes
		int persistent_slot; // index into launch_cache::persistent, or -1: not a persistent launch
		int per_cu_cap;		 // persistent launches: workgroups per CU at most
		uint32_t first_chunk; // a pass: the chunk of every pixel its items start at (queue.chunks is the PASS's chunk count); else 0
		// a frame that is NOT launched (RT_HIP_UNSUPPORTED with this text): traced boxes beyond box_max_count without a tree, or tables and chunk sums
		// beyond a workgroup's LDS (the box builds: workgroup_lds_bytes; every build: launch_request::lds_limit).  Empty: the plan stands.
		char refusal[192];
	};
	launch_plan plan_launch(const launch_request& request);
}
