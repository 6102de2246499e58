// rt_amd/csrc/kernels.hpp — host-visible launch interface of the gfx950 kernels (internal to librt_hip.so).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "launch_plan.hpp" // (the launch policy: queue_params, the thresholds, launch_plan)
#include "frame_setup.hpp" // (frame_params, the kernels' per-frame uniforms, and the host code that fills them)

namespace rt_hip
{
	// The scene resident in HBM.
	//   * the soagen columns exactly as the reference fills them at load (src/scene.cpp:583,595): the LDS-tiled
	//     kernel streams these, one coalesced dword per lane per column;
	//   * per-primitive tables derived from them at upload: (center, radius^2) / (normal, d) as float4, and the
	//     shading inputs of the primitive's material — (albedo.rgb * reflectivity, roughness) and a metal flag
	//     (mg_ray_tracer.cpp:115,131,142-152) — so that a hit needs one indexed lookup instead of two dependent ones;
	//   * the per-material shading table for kernels that only know the winning primitive's material index.
	// RT_HIP_FLAG_BVH: the sphere hierarchy of the resident scene (bvh.hpp), built on the host at the first such frame of a scene.
	// It lives in device memory (scene.hip, ensure_bvh) and reaches the BVH kernel through a pointer: device_scene, the other
	// kernels' argument, stays as it is.
	struct device_bvh
	{
		const float4* nodes;	// 4 per inner node
		const float4* spheres;	// (c, r^2) of the tree's spheres in leaf order
		const uint32_t* order;	// their indices in the scene
		const uint32_t* always; // indices of the spheres outside the tree (scanned linearly by every query)
		uint32_t root, n_tree, n_always;
		float cx, cy, cz, radius; // a ball around every tree sphere: the cull margin's C and R (bvh_scan.hpp)
	};

	struct device_scene
	{
		uint32_t n_spheres, n_planes, n_materials;
		const float* sphere_cx;
		const float* sphere_cy;
		const float* sphere_cz;
		const float* sphere_r;
		const uint32_t* sphere_material;
		const float* plane_nx;
		const float* plane_ny;
		const float* plane_nz;
		const float* plane_d;
		const uint32_t* plane_material;
		const float4* material_shading; // per material: (attenuation.rgb, roughness)
		const uint32_t* material_type;
		// derived per-primitive tables; spheres first, then planes (index n_spheres + i), then boxes (index n_spheres + n_planes + i: the
		// shading and scatter rows of the box's material, read under RT_HIP_FLAG_TRACE_BOXES; the geometry row is zero)
		const float4* primitive_geometry; // sphere: (cx, cy, cz, r*r); plane: (nx, ny, nz, d)
		const float4* primitive_shading;  // (attenuation.rgb, roughness) of the primitive's material
		const uint32_t* primitive_scatter; // scatter function of the primitive's material: scatter_lambert / scatter_metal
		// the same two tables under sm_ray_tracer's scatter table (RT_HIP_FLAG_SM_MATERIALS): dielectric, air, vacuum, water
		// and ice become scatter_dielectric, and their shading.w carries the reflectivity (= index of refraction)
		const float4* primitive_shading_sm;
		const uint32_t* primitive_scatter_sm;
		// the boxes as two float4 each — (min corner, material index as bits) and (max corner, 0), corners = center -/+ extents: read by
		// the preview (RT_HIP_FLAG_PREVIEW) and by the box builds of the render kernels (RT_HIP_FLAG_TRACE_BOXES) — and, for the preview
		// alone, the materials' plain albedo
		uint32_t n_boxes;
		const float4* box_bounds;
		const float4* material_albedo;
		// every plane normal is finite with components of at most 2^40 in magnitude (scene.hip; any scene rt's loader makes: it
		// normalises them).  A ray's direction is normalised, so n . d is then NaN, infinite (a degenerate direction) or below 2^60:
		// what lets the scalar-register kernels take a lone plane's 1 / (n . d) without a guard (scan.hpp, test_one_plane)
		uint32_t planes_tame;
	};

	enum : uint32_t
	{
		scatter_lambert = 0,	// mg_ray_tracer.cpp:110-123
		scatter_metal = 1,		// mg_ray_tracer.cpp:126-140
		scatter_dielectric = 2,	// sm_ray_tracer.cpp:181-219 (opt-in)
		scatter_emit = 3,		// a light (RT_HIP_FLAG_EMISSION): no scatter at all — the row's shading.rgb is the emission and the path ends; only
								// the light variant of the per-primitive tables holds it, and only the light builds read that
		scatter_emit_sampled = 4 // a SAMPLED light (RT_HIP_FLAG_DIRECT_LIGHT): scatter_emit, except that the segment behind a lambert vertex —
								// which has sampled the lights itself — finds it worth 0; only the direct variant of the scatter tables holds it
	};

	// RT_HIP_FLAG_DIRECT_LIGHT: the sampled-light list lies direct_list_bytes IN FRONT of the light variant's (mg) shading table, which the
	// direct builds are handed as device_scene::primitive_shading — found from that pointer, the way box_bvh_descriptor_offset works, so
	// that no kernel argument is added or moved.  A header of 256 bytes whose first word is n, then per sampled light two float4:
	// (centre.xyz, radius) and (emission.rgb, sphere index as bits).
	constexpr uint32_t direct_max_lights = 256; // (direct_light::max_sampled_lights)
	constexpr size_t direct_list_header_bytes = 256;
	constexpr size_t direct_list_bytes = direct_list_header_bytes + direct_max_lights * 2u * sizeof(float4);

	// the whole scene of the `small` kernel, passed by value as a kernel argument (-> SGPRs); host copy kept by the context
	// (scalar_max_spheres: launch_plan.hpp)
	struct small_scene
	{
		float4 geometry[scalar_max_spheres]; // spheres (center, radius^2), then planes (normal, d)
		float4 shading[scalar_max_spheres];	 // (attenuation.rgb, roughness or index of refraction) of the primitive's material
		uint32_t scatter[scalar_max_spheres]; // scatter_*
	};

	// What the big-scene kernels exchange chunk sums through (owned by the context, grown on demand), and what the other builds are handed
	// in the same two kernel arguments — render_queue has ONE argument block, which no build changes by a byte, so a value only some builds
	// need travels in a word those builds do not otherwise read.  WHICH BUILD READS WHICH WORD, the whole contract (packed on the host by
	// pack_words, kernels.hip; unpacked on the device by unpack_words, queue_build.hpp — nothing else casts these words):
	//   argument `item_sums`    rolling builds (scan_tiled, scan_streamed, scan_streamed_dense): item_sums.  scan_bvh and its pass / box /
	//                           light builds: `bvh`; scan_bvh_boxtree reads the box hierarchy's descriptor box_bvh_descriptor_offset bytes
	//                           behind it (box_bvh_scan.hpp).  Every other build: not read.
	//   argument `pixel_done`   rolling builds: pixel_done.  Pass and adaptive builds (scan_*_pass, scan_*_adapt): `accum`; the adaptive
	//                           builds find their state words and pass sums behind it (rt_hip.h, rt_hip_adaptive_pass_device).  Every
	//                           other build: not read.
	//   queue_params::block_items   rolling builds: items a wave draws at a time.  Pass and adaptive builds: launch_plan::first_chunk.
	//                           Every other build (tile-per-wave, no pass): launch_arguments::first_row, the image row the grid starts at —
	//                           0, or the height of the frame's sky band.
	struct rolling_buffers
	{
		// 16 bytes per item of this rank's rows (a chunk sum on its way to the lane that folds the pixel); not needed when a pixel is one
		// chunk.  With sub-chunk items: 16 bytes per SAMPLE
		unsigned long long* item_sums = nullptr;
		// one arrival counter per pixel; zeroed on the launch's own stream in front of every launch (render.hip)
		uint32_t* pixel_done = nullptr;
		// RT_HIP_FLAG_BVH: the hierarchy's descriptor in device memory (the BVH kernel keeps no sums in HBM); under RT_HIP_FLAG_BOX_BVH the
		// pair of descriptors (render.hip)
		const device_bvh* bvh = nullptr;
		// A pass of a progressive frame (launch_plan::build.pass; render_queue<scan_*_pass, ..>): the pixels' running sums, 3 floats per pixel
		// laid out like the float mean (the pass builds are tile-per-wave kernels, which have no arrival counters); an adaptive pass: the
		// block of accumulator, state words, pass sums and moments
		float* accum = nullptr;
	};

	struct device_counters
	{
		// path segments traced, as `segment_counters` partial sums (the host adds them up): every wave adds its count
		// once, and 130 000 atomics on ONE address serialise at about 12 ns each — more than a small launch takes
		static constexpr unsigned segment_counters = 64;
		unsigned long long segments[segment_counters];
		unsigned long long next_item; // head of the item sequence of the big-scene kernels; zeroed before every launch
#ifdef RT_HIP_REGION_COUNTERS
		static constexpr unsigned regions = 13; // experiment variant only (kernels.hip, RT_HIP_REGION)
		unsigned long long region_runs[regions], region_lanes[regions];
#endif
#ifdef RT_HIP_BVH_CHECK
		// experiment variant only (tools/bvh_sweep.py --check): sphere queries of the BVH kernel answered again by the linear scan,
		// and how many of them it answered differently (must stay 0)
		unsigned long long bvh_checked, bvh_disagreements;
#endif
#ifdef RT_HIP_WAVE_CLOCKS
		// experiment variant only (tools/gpu_wave_tail.py): when every wave of a persistent launch started, found the
		// tile queue dry and retired, in ticks of the constant 100 MHz clock (s_memrealtime)
		static constexpr unsigned clocked_waves = 16384;
		unsigned long long wave_clocks[clocked_waves][3];
#endif
	};

	// what a context remembers between launches: workgroups per CU that stay resident, for the persistent (big-scene) kernels
	struct launch_cache
	{
		struct entry
		{
			size_t lds_bytes = 0;
			int per_cu = 0;
		};
		entry persistent[persistent_cache_slots]; // indexed by launch_plan::persistent_slot
	};

	// what a render launch is made of: the caller has made `plan` (plan_launch) and prepared the buffers from the same plan
	struct launch_arguments
	{
		const frame_params& frame;
		const device_scene& scene; // (the light builds: a copy whose per-primitive shading / scatter pointers are the light variant's, render.hip)
		const small_scene& small;  // valid when the plan's variant is RT_HIP_KERNEL_SMALL; tables already chosen by flag
		const launch_plan& plan;
		uint32_t* d_rgba8;
		float* d_rgb_f32;
		device_counters* d_counters;
		const rolling_buffers& rolling; // big scenes: sized as the plan says, pixel_done zeroed in front of the launch
		uint32_t compute_units;			// of the device: the big-scene kernels are launched persistent
		launch_cache& cache;
		hipStream_t stream;
		uint32_t first_row = 0; // a tile-per-wave launch that is no pass: the image row its grid starts at (the rows under a sky band; frame.local_rows is then the frame's height)
	};

	// launches what the plan says; returns the kernel variant launched (RT_HIP_KERNEL_*)
	uint32_t launch_render(const launch_arguments& a);

	// the same with RT_HIP_FLAG_FAST's arithmetic (kernels.hip built with RT_HIP_FAST_BUILD); mg scatter table only
	uint32_t launch_render_fast(const launch_arguments& a);

	// the sky band (sky_band.hip): rows [0, band.local_rows) of a frame, every sample of which is one segment that ends in the sky
	void launch_sky_band(const frame_params& band, uint32_t* d_rgba8, float* d_rgb_f32, device_counters* d_counters, hipStream_t stream);

	// RT_HIP_FLAG_PREVIEW: one ray per pixel, reference src/renderers/rasterizer.cpp:24-85
	void launch_preview(const frame_params& frame, const device_scene& scene, uint32_t* d_rgba8, float* d_rgb_f32, device_counters* d_counters, hipStream_t stream);

	// `width` in 32-bit words per row (pixels, or 3 x pixels for the float mean)
	void launch_assemble(uint32_t width,
						 uint32_t height,
						 uint32_t world,
						 uint32_t stripe_rows,
						 uint32_t padded_local_rows,
						 const uint32_t* d_gathered,
						 uint32_t* d_frame,
						 uint32_t first_rank,		// rows of ranks below this one are left alone (already in the frame)
						 bool frame_is_host_memory, // the caller's page-locked back buffer: system-scope stores
						 hipStream_t stream);
}
