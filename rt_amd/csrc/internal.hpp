// rt_amd/csrc/internal.hpp — what the translation units of librt_hip.so share: the context, error translation, the
// grow-only device / page-locked buffers, and the functions one unit offers the others.
//
//   context.hip   library entry points, create / destroy, multi-GPU and rank contexts, RCCL and frame-group joins
//   scene.hip     the caller's columns: checks, fingerprint, the HBM image, residency
//   frame.hip     the caller's frame buffer: the module-owned page-locked frame and its delivery threads (the default),
//                 the opt-in page-lock of the caller's own buffer, NUMA placement
//   render.hip    one launch (rt_hip_render_device), the work counters, the single-GPU drop-in rt_hip_render
//   frame_call.hip   the steps the single-context drop-in calls share: the scene prologue, the frame key, the drain-then-abandon
//                 scope, and the two ways a finished frame reaches the caller's plain memory, carried and staged
//   frame_setup.cpp, launch_plan.cpp   (host compiler, no HIP) what a launch is refused for, its per-frame constants, its plan
//   passes.hip    a frame in resumable passes: rt_hip_render_progressive (sequencing: progressive.cpp, host compiler; one pass at the
//                 device level, rt_hip_render_pass_device, is render.hip's)
//   denoise.hip   the guide-buffer denoiser: its two kernels, rt_hip_guide_device, rt_hip_denoise_device and
//                 rt_hip_denoise_progressive (parameters: denoise.cpp, host compiler; per-pixel rules: denoise_rules.hpp)
//   adaptive.hip  adaptive sampling: adaptive_update, rt_hip_adaptive_update_device, rt_hip_adaptive_pass_device and the drop-in
//                 rt_hip_render_adaptive (parameters, sequencing: adaptive.cpp, host compiler; per-pixel rules: adaptive_rules.hpp)
//   temporal.hip  temporal accumulation: reproject_frame, rt_hip_reproject_device and the drop-in rt_hip_render_temporal
//                 (parameters, the forward matrix, same_history: temporal.cpp, host compiler; per-pixel rule: reproject_rules.hpp)
//   upsample.hip  guided upsampling: upsample_frame, rt_hip_upsample_device and the drop-in rt_hip_render_upscaled
//                 (parameters, sizes: upsample.cpp, host compiler; per-pixel rules: upsample_rules.hpp)
//   tonemap.hip   tone mapping: luminance_histogram, exposure_from_histogram, tonemap_frame, rt_hip_tonemap_device and the
//                 drop-in rt_hip_render_tonemapped (parameters, the spec parser: tonemap.cpp, host compiler; per-element rules: tonemap_rules.hpp)
//   bloom.hip     bloom: bloom_prefilter, bloom_down, bloom_up, bloom_composite, rt_hip_bloom_device and the drop-in
//                 rt_hip_render_bloomed (parameters, the level plan, the spec parser: bloom.cpp, host compiler; per-element rules: bloom_rules.hpp)
//   multi.hip     rt_hip_render on several GPUs: stripes, one gather, assemble
//   group.hip     rt_hip_render as one rank of a frame group (rank processes storing into one shared back buffer)
//   kernels.hip   the gfx950 kernels (compiled twice: parity contract and RT_HIP_FLAG_FAST arithmetic)
//
// Everything here has hidden visibility: the library exports the C entry points of include/rt_hip.h and nothing else.
// The test-only library librt_hip_kat.so (kat.hip, kat_kernels.hip) includes this header for the LAYOUT of rt_hip_ctx —
// it reads a context's device and resident scene — and calls nothing of librt_hip.so that is not in rt_hip.h.
#pragma once

#include "../../include/rt_hip.h"
#include "contract.hpp"
#include "delivery.hpp"
#include "frame_group.hpp"
#include "kernels.hpp"
#include "progressive.hpp"
#include "adaptive.hpp"
#include "lights.hpp"
#include "lens.hpp"
#include "sky_band.hpp"

#include <rccl/rccl.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

namespace rt_hip
{
	// ---- error translation: no exception and no HIP error code crosses the C boundary (src/renderer.hpp:11: noexcept) ----
	rt_hip_status fail(rt_hip_status status, const char* format, ...) __attribute__((format(printf, 2, 3)));
	const std::string& last_error();
	inline rt_hip_status ok() { return RT_HIP_OK; }

#define RT_HIP_TRY_NCCL(expr)                                                                                          \
	do                                                                                                                 \
	{                                                                                                                  \
		const ncclResult_t rt_hip_try_res = (expr);                                                                    \
		if (rt_hip_try_res != ncclSuccess)                                                                             \
			return ::rt_hip::fail(RT_HIP_RUNTIME_ERROR, "%s failed: %s", #expr, ncclGetErrorString(rt_hip_try_res));   \
	}                                                                                                                  \
	while (false)

#define RT_HIP_TRY(expr)                                                                                               \
	do                                                                                                                 \
	{                                                                                                                  \
		const hipError_t rt_hip_try_err = (expr);                                                                      \
		if (rt_hip_try_err != hipSuccess)                                                                              \
			return ::rt_hip::fail(RT_HIP_RUNTIME_ERROR, "%s failed: %s", #expr, hipGetErrorString(rt_hip_try_err));    \
	}                                                                                                                  \
	while (false)

	// grow-only device allocation
	struct device_buffer
	{
		void* ptr = nullptr;
		size_t bytes = 0;

		hipError_t reserve(size_t wanted)
		{
			if (wanted <= bytes)
				return hipSuccess;
			if (ptr)
			{
				(void)hipFree(ptr);
				ptr = nullptr;
				bytes = 0;
			}
			const hipError_t e = hipMalloc(&ptr, wanted);
			if (e == hipSuccess)
				bytes = wanted;
			return e;
		}
		void release()
		{
			if (ptr)
				(void)hipFree(ptr);
			ptr = nullptr;
			bytes = 0;
		}
		template <typename T>
		T* as() const
		{
			return static_cast<T*>(ptr);
		}
	};

	// grow-only page-locked HOST allocation owned by the module (hipHostMalloc: mapped into every device's address space).
	// Whatever the HIP runtime reads from or writes to host memory on this module's behalf is one of these — never the
	// caller's pageable memory, and never a pageable block of the module's own (see frame.hip, "Why the module stages").
	struct pinned_buffer
	{
		void* ptr = nullptr;
		size_t bytes = 0;

		hipError_t reserve(size_t wanted)
		{
			if (wanted <= bytes)
				return hipSuccess;
			release();
			// a little slack, so that a window dragged larger pixel row by pixel row does not re-allocate every frame
			const size_t rounded = (wanted + wanted / 8u + 4095u) & ~static_cast<size_t>(4095u);
			const hipError_t e = hipHostMalloc(&ptr, rounded, hipHostMallocMapped | hipHostMallocPortable);
			if (e == hipSuccess)
				bytes = rounded;
			else
				ptr = nullptr;
			return e;
		}
		void release()
		{
			if (ptr)
				(void)hipHostFree(ptr);
			ptr = nullptr;
			bytes = 0;
		}
		template <typename T>
		T* as() const
		{
			return static_cast<T*>(ptr);
		}
	};

	inline double seconds_since(std::chrono::steady_clock::time_point t0)
	{
		return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
	}

	inline float elapsed_or_zero(hipEvent_t from, hipEvent_t to)
	{
		float ms = 0.0f;
		if (hipEventElapsedTime(&ms, from, to) != hipSuccess)
		{
			(void)hipGetLastError();
			ms = 0.0f;
		}
		return ms;
	}

	// what the denoiser keeps on a context (denoise.hip): everything is grown on demand and freed with the context
	struct denoise_state
	{
		device_buffer scratch[2];	  // the image between two iterations: 12 bytes per pixel each, ping-pong
		device_buffer mean, filtered; // rt_hip_denoise_progressive: accumulator / samples_done, and the filter's float result
		device_buffer packed;		  // ... and its packed pixels
		device_buffer guide;		  // ... and the guide of the accumulation in flight, kept while `guide_key` is the accumulation's
		pinned_buffer staging;		  // the results' landing place on the host
		frame_key guide_key{};
		bool have_guide = false;
		hipEvent_t begin = nullptr, end = nullptr; // device time of guide + filter
		void release()
		{
			for (device_buffer* b : { &scratch[0], &scratch[1], &mean, &filtered, &packed, &guide })
				b->release();
			staging.release();
			for (hipEvent_t* e : { &begin, &end })
			{
				if (*e)
					(void)hipEventDestroy(*e);
				*e = nullptr;
			}
			have_guide = false;
		}
	};

	// what temporal accumulation keeps on a context (temporal.hip): everything is grown on demand and freed with the context
	struct temporal_state
	{
		device_buffer rgb[2], record[2]; // the history, ping-pong: 12 + 32 bytes per pixel a set
		device_buffer traced, guide;	 // the frame's traced float mean and its guide
		device_buffer filtered, packed;	 // the spatial filter's float result, and the packed pixels
		device_buffer found;			 // one word: the pixels that found history
		pinned_buffer staging;			 // the results' landing place on the host
		bool have_history = false;		 // set `current` holds a history made under `key`
		uint32_t current = 0;
		uint32_t frames = 0;			 // frames blended into it so far
		frame_key key{};
		hipEvent_t end = nullptr;		 // behind guide + reprojection + filter (frames that keep stats)
		void release()
		{
			for (device_buffer* b : { &rgb[0], &rgb[1], &record[0], &record[1], &traced, &guide, &filtered, &packed, &found })
				b->release();
			staging.release();
			if (end)
				(void)hipEventDestroy(end);
			end = nullptr;
			have_history = false;
			frames = 0;
		}
	};

	// what rt_hip_render_upscaled keeps on a context (upsample.hip): everything is grown on demand and freed with the context
	struct upscale_state
	{
		device_buffer low_mean, low_packed, low_filtered; // the traced low frame: float mean, the packed pixels its launch writes, the filter's result
		device_buffer guide_low, guide_full;			  // the guide at the two sizes
		device_buffer rgb, packed;						  // the rebuilt frame: float mean (when asked for) and packed pixels
		device_buffer orphans;							  // one word
		pinned_buffer staging;							  // the results' landing place on the host
		hipEvent_t end = nullptr;						  // behind guides + filter + upsampling (frames that keep stats)
		void release()
		{
			for (device_buffer* b : { &low_mean, &low_packed, &low_filtered, &guide_low, &guide_full, &rgb, &packed, &orphans })
				b->release();
			staging.release();
			if (end)
				(void)hipEventDestroy(end);
			end = nullptr;
		}
	};

	// what tone mapping keeps on a context (tonemap.hip): everything is grown on demand and freed with the context
	struct tonemap_state
	{
		device_buffer histogram;   // the meter's 256 bins and the skipped count (rt_hip_tonemap_device's too)
		device_buffer traced;	   // rt_hip_render_tonemapped: the traced float mean, mapped in place
		device_buffer packed;	   // ... the packed pixels (the traced frame's own, then the mapped ones)
		device_buffer record;	   // ... the 8-word state record, kept from call to call
		uint32_t width = 0, height = 0; // ... the frame the record was kept for (0: none)
		pinned_buffer staging;	   // the results' landing place on the host
		hipEvent_t end = nullptr;  // behind the three launches (frames that keep stats)
		void release()
		{
			for (device_buffer* b : { &histogram, &traced, &packed, &record })
				b->release();
			staging.release();
			if (end)
				(void)hipEventDestroy(end);
			end = nullptr;
			width = height = 0;
		}
	};

	// what bloom keeps on a context (bloom.hip): everything is grown on demand and freed with the context
	struct bloom_state
	{
		device_buffer pyramid;	   // every level back to back, 12 bytes a texel (rt_hip_bloom_device's too)
		device_buffer traced;	   // rt_hip_render_bloomed: the traced float mean, bloomed and mapped in place
		device_buffer packed;	   // ... the packed pixels (the traced frame's own, then the mapped ones)
		device_buffer record;	   // ... tone mapping's 8-word state record, kept from call to call: NOT rt_hip_render_tonemapped's
		uint32_t width = 0, height = 0; // ... the frame the record was kept for (0: none)
		pinned_buffer staging;	   // the results' landing place on the host
		hipEvent_t end = nullptr;  // behind the last launch (frames that keep stats)
		void release()
		{
			for (device_buffer* b : { &pyramid, &traced, &packed, &record })
				b->release();
			staging.release();
			if (end)
				(void)hipEventDestroy(end);
			end = nullptr;
			width = height = 0;
		}
	};

	// what adaptive sampling keeps on a context (adaptive.hip): everything is grown on demand and freed with the context
	struct adaptive_accumulation
	{
		adaptive_state state;		 // the accumulation in flight (adaptive.hpp)
		device_buffer block;		 // accum, state, pass_sum, moments: 36 bytes per pixel (rt_hip.h, rt_hip_adaptive_pass_device)
		device_buffer active;		 // one word: the pixels still active after the last pass
		device_buffer scratch;		 // the update kernel's output words on their way back (12 bytes per pixel; the device-level call's too)
		pinned_buffer staging;		 // the results' landing place on the host
		pinned_buffer traced;		 // one word: the pixels the last rt_hip_adaptive_pass_device traced, for its stats
		uint32_t traced_pass_samples = 0; // != 0: the most recent launch was that call's, a pass of so many samples (render_device clears it)
		std::vector<uint32_t> frame; // the complete frame, kept on the host for calls that come after it
		hipEvent_t end = nullptr;	 // behind the update (passes that keep stats)
		void release()
		{
			for (device_buffer* b : { &block, &active, &scratch })
				b->release();
			staging.release();
			traced.release();
			traced_pass_samples = 0;
			if (end)
				(void)hipEventDestroy(end);
			end = nullptr;
			state = adaptive_state{};
			frame.clear();
		}
	};

	struct frame_delivery; // below: the module-owned frame and the threads that carry it to the caller's buffer

	// (RT_HIP_FLAG_PERSISTENT_FRAME and RT_HIP_FLAG_STATS are rt_hip_render's own: they do not travel to the launch)
	constexpr uint32_t render_flag_mask = RT_HIP_FLAG_FORCE_TILED | RT_HIP_FLAG_FORCE_RESIDENT | RT_HIP_FLAG_SM_MATERIALS | RT_HIP_FLAG_PREVIEW | RT_HIP_FLAG_FORCE_STREAMED | RT_HIP_FLAG_FAST | RT_HIP_FLAG_FORCE_HALF_CHUNKS | RT_HIP_FLAG_FORCE_WHOLE_CHUNKS | RT_HIP_FLAG_BVH | RT_HIP_FLAG_BVH_DEVICE_BUILD | RT_HIP_FLAG_TRACE_BOXES | RT_HIP_FLAG_BOX_BVH | RT_HIP_FLAG_EMISSION | RT_HIP_FLAG_DIRECT_LIGHT | RT_HIP_FLAG_THIN_LENS;

}

struct rt_hip_ctx
{
	int device = 0;
	uint32_t compute_units = 256;
	size_t workgroup_lds_bytes = 0; // LDS bytes one workgroup may ask for, as the device's properties say (rt_hip_create); 0 = unknown
	int numa_node = -1; // host NUMA node the GPU hangs off (sysfs), -1 = unknown

	// the scene, resident in HBM: one buffer holding every column back to back (256-byte aligned starts)
	rt_hip::device_buffer scene_columns;
	rt_hip::pinned_buffer scene_staging; // host image of that block on its way up (built here, copied from here)
	rt_hip::device_scene scene{};
	rt_hip::small_scene small{}, small_sm{}; // host copies of the kernel-argument scene of the `small` kernel (mg / sm scatter tables)
	bool have_scene = false;
	uint32_t samples_per_pixel = 0, max_bounces = 0;
	float inverse_view_projection[16]{};

	// big scenes: chunk sums on their way between waves and the pixels' arrival counters (kernels.hpp, rolling_buffers)
	rt_hip::device_buffer item_sums, pixel_done;
	rt_hip::device_buffer counters;
	rt_hip::device_counters* counters_host = nullptr; // page-locked; filled by an asynchronous copy right behind every launch that keeps stats
	hipEvent_t render_begin = nullptr, render_end = nullptr, counters_copied = nullptr;
	bool render_recorded = false; // the most recent launch was bracketed by the events above and its counters were read back
	bool launched = false;		  // something has been launched on last_stream
	hipStream_t last_stream = nullptr;
	// exchange phases of a multi-GPU frame on the root's stream (frames that keep stats): stripes on the root, frame
	// assembled, frame copied to the host
	hipEvent_t gathered = nullptr, assembled = nullptr, copied = nullptr;
	rt_hip_phases phases{};
	rt_hip::launch_cache cache; // what the launch code remembers per context (occupancy of the persistent kernels)

	// the context's own stream: everything rt_hip_render() enqueues goes here (never the process-wide null stream)
	hipStream_t stream = nullptr;

	// ---- several GPUs behind one render() (rt_hip_create_multi) ----
	// The context the caller holds is member 0 (the root); it owns members 1 .. n-1, one per further device.
	bool multi = false;
	bool peer_copy = false;			  // RT_HIP_MULTI_PEER_COPY
	bool direct_frame = false;		  // RT_HIP_MULTI_DIRECT_FRAME
	// the renderer's ranks: `world` in all, of which this process holds first_rank .. first_rank + members - 1
	// (rt_hip_create_multi: all of them; rt_hip_create_rank: exactly one, the others live in other processes)
	uint32_t world = 1, first_rank = 0;
	std::vector<rt_hip_ctx*> peers;	  // members 1 .. n-1
	std::vector<ncclComm_t> comms;	  // one communicator per member, rank order (empty with peer_copy)
	rt_hip::device_buffer stripes_rgba, stripes_rgb;   // this member's compact stripe buffers (the gather's send side)
	rt_hip::device_buffer gathered_rgba, gathered_rgb; // root: n x padded stripes, rank order (the gather's receive side)
	hipEvent_t stripes_ready = nullptr;				   // recorded on `stream` after this member's launch (peer copies wait for it)
	// ---- or: one rank of a renderer whose ranks are processes that all map the caller's back buffer (rt_hip_join_frame_group)
	std::unique_ptr<rt_hip::frame_group> group;

	// ---- the frame's way to the caller (frame.hip) ----
	// Default: the module's OWN page-locked, mapped frame — the kernels store finished pixels straight into it — and a few
	// host threads that carry the pixels on into the caller's buffer while the rest of the frame is still being traced.
	std::unique_ptr<rt_hip::frame_delivery> delivery;
	rt_hip::device_buffer frame_rgb;	 // the float mean of the whole frame in HBM (optional second output)
	rt_hip::pinned_buffer staging_rgb;	 // ... and its landing place on the host
	uint64_t scene_fingerprint = 0;		 // of the caller's columns last uploaded: rt has no scene version counter (src/main.cpp:233-311)
	uint64_t scene_uploads = 0;			 // scenes made resident so far (scene.hip): what the sphere hierarchy below was built for
	uint64_t bvh_built_for = 0;			 // ... its scene_uploads when built (0 = none)
	rt_hip::device_buffer bvh_block;	 // RT_HIP_FLAG_BVH: descriptor, nodes, leaf-ordered spheres, their indices, the always list
	const rt_hip::device_bvh* bvh_descriptor = nullptr; // ... its first bytes: what the BVH kernel is handed (rolling_buffers::bvh)
	bool bvh_device_built = false;		 // ... and which builder made it: bvh_build.hip (RT_HIP_FLAG_BVH_DEVICE_BUILD) or bvh.cpp
	rt_hip::device_buffer bvh_scratch;	 // the device builder's keys, ping-pong buffers and level queues
	// RT_HIP_FLAG_BOX_BVH (scene.hip, ensure_box_bvh): a copy of the sphere hierarchy's descriptor, the box hierarchy's descriptor
	// box_bvh_descriptor_offset bytes behind it, then nodes, leaf-ordered corners, their indices, the always list.  What the
	// scan_bvh_boxtree build is handed in rolling_buffers::bvh's place.
	rt_hip::device_buffer box_bvh_block;
	uint64_t box_columns_print = 0;		 // fingerprint of the resident box_bounds pairs (make_resident)
	uint64_t box_bvh_print = 0;			 // ... of the pairs the tree in box_bvh_block was built from
	uint32_t box_bvh_count = 0;			 // ... and how many they were
	bool box_bvh_built = false;
	uint64_t box_bvh_sphere_stamp = 0;	 // which sphere hierarchy the copied descriptor describes (0 = none): 2 * bvh_built_for + bvh_device_built
	uint64_t box_bvh_builds = 0;		 // host builds so far (the known-answer library reads it: tests/test_gpu_box_bvh.py)
	size_t scene_bytes = 0;				 // size of the resident block
	// RT_HIP_FLAG_EMISSION: the emission table (rt_hip_set_emission: context state, survives scene uploads) and the
	// LIGHT variant of the four per-primitive shading / scatter tables derived from it and the resident scene (scene.hip,
	// ensure_light_tables): a light's primitives carry (emission.rgb, 0) and scatter_emit, every other row is the ordinary table's.
	// Built when a frame with the flag finds them missing or stale — after a scene upload, after rt_hip_set_emission — and handed to
	// the light builds in a COPY of `scene` whose four pointers point here (render.hip): no kernel argument is added or moved.
	std::vector<float> emission;		 // 3 floats per row
	bool have_emission = false;
	uint32_t emission_rows = 0, emission_lights = 0; // rows of the table, and how many of them are lights
	uint64_t emission_version = 0;		 // rt_hip_set_emission calls so far
	rt_hip::device_buffer light_tables;	 // shading, scatter, shading_sm, scatter_sm (256-byte aligned starts)
	uint64_t light_tables_uploads = 0, light_tables_version = 0; // the scene_uploads and emission_version they were built for (0 = none)
	const float4* light_shading = nullptr;
	const uint32_t* light_scatter = nullptr;
	const float4* light_shading_sm = nullptr;
	const uint32_t* light_scatter_sm = nullptr;
	// RT_HIP_FLAG_DIRECT_LIGHT: the SAMPLED-LIGHT LIST lies in the same block, in FRONT of the light variant's shading table
	// (direct_list_bytes before light_shading: a count word, then two float4 per sampled light — the direct builds find it from the
	// variant pointer, kernels.hpp), built and invalidated with the tables.  The scatter tables exist a second time with
	// scatter_emit_sampled in the sampled lights' rows: the frames of RT_HIP_FLAG_EMISSION alone go on reading the tables above.
	uint32_t sampled_lights = 0; // n of the resident scene under the table (valid with the tables)
	const uint32_t* light_scatter_direct = nullptr;
	const uint32_t* light_scatter_sm_direct = nullptr;
	// RT_HIP_FLAG_THIN_LENS: the lens (rt_hip_set_lens: context state, survives scene uploads).  A frame with the flag and an
	// aperture derives its ten words from it and the frame's matrix (lens.cpp) and hands them to the lens builds in frame_params words only
	// the homogeneous camera form reads (render.hip): no kernel argument is added or moved.
	rt_hip_lens lens{};
	bool have_lens = false;
	// Opt-in (RT_HIP_FLAG_PERSISTENT_FRAME, frame groups): the CALLER's buffer, page-locked and mapped into the GPU's address
	// space while it keeps arriving at the same address: the kernel renders straight into it.  The caller then owes the
	// module rt_hip_forget_frame before that memory is unmapped (rt_hip.h).
	void* pinned_frame = nullptr;
	size_t pinned_bytes = 0;
	void* refused_frame = nullptr; // a buffer whose page-lock failed: not tried again while it keeps arriving
	size_t refused_bytes = 0;

	const void* asked_pointer = nullptr; // rt_hip_render_device: the last output pointer and whether it is host memory
	bool asked_pointer_is_host = false;

	rt_hip_stats stats{};

	// ---- a frame in passes (rt_hip_render_progressive, passes.hip) ----
	rt_hip::pass_state progressive;			  // the accumulation in flight
	uint32_t progressive_passes = 0;		  // passes launched for it so far
	rt_hip::device_buffer accum;			  // the pixels' running sums: 3 floats per pixel, kept from pass to pass
	std::vector<uint32_t> progressive_frame;  // the finished frame, kept on the host for calls that come after the last pass
	rt_hip::denoise_state denoise;			  // the denoiser's scratch images and the kept guide (denoise.hip)
	rt_hip::temporal_state temporal;		  // the history of rt_hip_render_temporal (temporal.hip)
	rt_hip::adaptive_accumulation adaptive;	  // the accumulation of rt_hip_render_adaptive (adaptive.hip)
	rt_hip::upscale_state upscale;			  // the scratch of rt_hip_render_upscaled (upsample.hip)

	// ---- the sky band (sky_band.hpp, render.hip) ----
	bool sky_band_enabled = true;		 // RT_HIP_SKY_BAND=0 in the environment at creation: no frame of this context takes a band
	bool sky_band_log = false;			 // RT_HIP_SKY_BAND_LOG=1 at creation: one line per launch on stderr with the band's rows
	std::vector<float> sphere_table;	 // host copy of the resident scene's (c, r^2) rows (scene.hip; empty beyond sky_band_max_spheres)
	// the rule's last answer and what it was asked: the resident scene, the launch's flags and kernel, the frame's constants without its seed
	struct
	{
		bool valid = false;
		uint64_t scene_uploads = 0;
		uint32_t flags = 0;
		int scan = 0;
		rt_hip::frame_params frame{};
		uint32_t rows = 0;
	} sky_band_asked;

	// ---- tone mapping (tonemap.hip) ----
	rt_hip::tonemap_state tonemap; // the meter's histogram and the scratch of rt_hip_render_tonemapped
	rt_hip::bloom_state bloom;	   // the pyramid and the scratch of rt_hip_render_bloomed

	rt_hip_ctx() = default;
	rt_hip_ctx(const rt_hip_ctx&) = delete;
	rt_hip_ctx& operator=(const rt_hip_ctx&) = delete;
};

namespace rt_hip
{
	// ---- context.hip ----
	rt_hip_ctx* member_of(rt_hip_ctx* ctx, int rank);

	// ---- scene.hip ----
	// layout of the single HBM block: every column starts on a 256-byte boundary.  A function of the four counts alone.
	struct scene_layout
	{
		size_t scx, scy, scz, sr, sm;				 // sphere columns
		size_t pnx, pny, pnz, pd, pm;				 // plane columns
		size_t shading, type;						 // per material
		size_t geometry, prim_shading, prim_metal;	 // derived per-primitive tables (spheres, then planes, then boxes: of a box only its material's entries mean anything)
		size_t prim_shading_sm, prim_scatter_sm;	 // the same under sm_ray_tracer's scatter table
		size_t box_bounds, albedo;					 // the boxes' corners (the preview, RT_HIP_FLAG_TRACE_BOXES); what only the preview reads
		size_t total;
	};
	// One render()'s view of the caller's scene: pointers checked, fingerprint taken once — shared by all members of a
	// multi-GPU context — and the image of the HBM block, which is built (in the first member's page-locked staging
	// buffer) only if some member turns out not to hold these columns yet.
	struct scene_request
	{
		const rt_hip_scene* scene = nullptr;
		scene_layout layout{};
		uint64_t print = 0;
		bool indices_checked = false;
		const unsigned char* image = nullptr; // page-locked host image of the block (one H2D copy per member that needs it)
		small_scene small{}, small_sm{};	  // the kernel-argument scene of the `small` kernel (mg / sm scatter tables)
	};
	rt_hip_status open_request(scene_request& r, const rt_hip_scene* scene);
	// Make `ctx` hold the request's scene (leaves ctx->device current)
	rt_hip_status make_resident(rt_hip_ctx* ctx, scene_request& r);
	// RT_HIP_FLAG_BVH: the resident scene's sphere hierarchy (scene.hip).  device_build: RT_HIP_FLAG_BVH_DEVICE_BUILD — built by
	// bvh_build.hip on `stream`, the stream the frame is about to be launched on; wait: the frame keeps stats, upload_ms is to hold the build
	rt_hip_status ensure_bvh(rt_hip_ctx* ctx, bool device_build, hipStream_t stream, bool wait);
	// RT_HIP_FLAG_BOX_BVH: make ctx->box_bvh_block hold the box hierarchy of the resident scene — built on the host (box_bvh.cpp) at
	// the first such frame after the box columns' fingerprint changed, its time added to upload_ms — behind a copy of the CURRENT
	// sphere hierarchy's descriptor (ensure_bvh has run), refreshed on `stream` whenever that hierarchy was rebuilt
	rt_hip_status ensure_box_bvh(rt_hip_ctx* ctx, hipStream_t stream);
	// RT_HIP_FLAG_EMISSION: make ctx->light_* the light variant of the resident scene's per-primitive tables under the context's emission
	// table (whose row count the caller has checked against the scene's materials); rebuilt only when the scene or the table is new
	rt_hip_status ensure_light_tables(rt_hip_ctx* ctx);

	// ---- render.hip ----
	// whole_frame_buffers: d_rgba8 / d_rgb_f32 are the whole width x height frame and every pixel goes to its image row
	// (several GPUs rendering into one host frame); otherwise the rank's compact stripe buffer, as the public call documents.
	// keep_stats: bracket the launch with timing events, zero the work counters before it and read them back after it.  Without
	// it NOTHING but the kernel is enqueued (the plug-in's call: rt_hip_render with stats == NULL).
	// host_frame: d_rgba8 is page-locked host memory (a mapped frame): the tiles are cut for PCIe writes (choose_queue).
	// pass: one pass of a progressive frame instead of the whole frame (NULL: the whole frame, as ever)
	// sky_band: the caller renders one whole frame in this one launch and takes a sky band where the rule finds one (rt_hip_render's
	// single-GPU path and rt_hip_render_device; the multi-GPU, frame-group, progressive, adaptive, temporal and denoise paths do not)
	struct render_pass
	{
		uint32_t first_sample, n_samples; // whole chunks, or up to the scene's samples_per_pixel (checked by the caller)
		float* d_accum;					  // the pixels' running sums, laid out like d_rgb_f32
		bool adaptive = false;			  // an adaptive pass (adaptive.hip): d_accum is the whole block — accum, state, pass_sum, moments — and no pixel is stored
	};
	rt_hip_status render_device(rt_hip_ctx* ctx, uint32_t width, uint32_t height, uint64_t seed, uint32_t flags, const rt_hip_partition* part, uint32_t* d_rgba8, float* d_rgb_f32, void* stream, bool whole_frame_buffers, bool keep_stats, bool host_frame,
								const render_pass* pass = nullptr, bool sky_band = false);
	rt_hip_status fetch_member_stats(rt_hip_ctx* ctx);
	rt_hip_stats stats_of_group_rank(const rt_hip_ctx* ctx, uint32_t rank);
	void sum_group_stats(const rt_hip_ctx* ctx, rt_hip_stats* out);

	// ---- denoise.hip (what temporal.hip uses of it) ----
	constexpr uint32_t max_frame_side = 1u << 15; // (a pixel's coordinates are int32 in the rules; rt's window is far below)
	// the name of a flag the guide does not take ("unknown flag bits" for a bit without a name); NULL: all accepted
	const char* refused_guide_flag(uint32_t flags);
	bool buffers_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes);
	// the constants centre_ray() (centre_ray.hpp) reads for a whole width x height frame seen through `matrix`
	frame_params centre_frame_params(uint32_t width, uint32_t height, const float* matrix);
	// the guide of the resident scene seen through `matrix`, and the a-trous filter, on device buffers: everything checked by the caller,
	// ctx->device current
	rt_hip_status launch_guide(rt_hip_ctx* ctx, uint32_t width, uint32_t height, const float* matrix, bool trace_boxes, float* d_guide, hipStream_t stream);
	rt_hip_status launch_filter(rt_hip_ctx* ctx, uint32_t width, uint32_t height, const float* d_in, const float* d_guide, const rt_hip_denoise_params& params, float* d_out, uint32_t* d_rgba, hipStream_t stream);

	// ---- tonemap.hip (what bloom.hip uses of it) ----
	// `params`, or the defaults; refused with the field's name behind `who`
	rt_hip_status resolve_tonemap(const char* who, const rt_hip_tonemap_params* params, rt_hip_tonemap_params& out);
	// the tone-mapping launches on device buffers (everything checked by the caller; ctx->device current)
	rt_hip_status launch_tonemap(rt_hip_ctx* ctx, uint32_t width, uint32_t height, const float* d_in, const rt_hip_tonemap_params& p, uint32_t* d_state, float* d_out, uint32_t* d_rgba, hipStream_t stream);

	// ---- multi.hip / group.hip ----
	rt_hip_status render_multi(rt_hip_ctx* root, const rt_hip_scene* scene, uint32_t* pixels_rgba8888, uint32_t width, uint32_t height, uint64_t seed, uint32_t flags, float* rgb_f32, rt_hip_stats* stats, std::chrono::steady_clock::time_point entered);
	rt_hip_status render_group(rt_hip_ctx* ctx, const rt_hip_scene* scene, uint32_t* pixels_rgba8888, uint32_t width, uint32_t height, uint64_t seed, uint32_t flags, float* rgb_f32, rt_hip_stats* stats, std::chrono::steady_clock::time_point entered);

	// ---- frame.hip ----
	int numa_node_of(int device);
	bool debug_frame();
	void place_stripes(void* ptr, size_t bytes, uint32_t width, uint32_t height, uint32_t stripe_rows, const std::vector<int>& node_of_rank);
	void unpin_frame(rt_hip_ctx* ctx);
	// `pin`: RT_HIP_FLAG_PERSISTENT_FRAME — page-lock the caller's buffer on first sight, keep the lock while the same buffer
	// keeps arriving; any other buffer (or no flag) first drops the old registration.  `stripe_nodes` (with the frame's
	// shape): place the row stripes on their owners' nodes instead of the whole buffer on this context's.
	void track_frame_buffer(rt_hip_ctx* ctx, uint32_t* pixels, size_t bytes, bool pin, bool may_move_pages = true, const std::vector<int>* stripe_nodes = nullptr, uint32_t width = 0, uint32_t height = 0);
	// page-locks on callers' memory this process holds right now (rt_hip_live_frame_locks)
	uint32_t live_frame_locks();

	// The module-owned frame of a context and its delivery to the caller's buffer (delivery.hpp has the idea).  Per frame:
	//   begin    the staging frame is in place (all zero) and the carrier's threads are looking at it; returns the frame as
	//            the current device sees it (the kernels' output pointer)
	//   ... launches that store packed pixels into it, hipStreamSynchronize ...
	//   finish   everything the device stored is visible: the rest of the frame is carried over; returns when every pixel
	//            is in the caller's buffer
	//   abandon  instead of finish, on any failure: nothing further is copied, the staging frame is wiped before its next use
	// The module-owned frame itself: anonymous memory of the module's own, placed on the host NUMA node the GPU hangs off
	// BEFORE it is first touched, then page-locked and mapped for every device (hipHostRegister: portable).  Not hipHostMalloc:
	// that puts the pages wherever the runtime likes; the module knows the node (sysfs), owns the memory and keeps the
	// carrier's helper threads on that node's CPUs, so frame, pollers and GPU sit on one socket (with the helpers left to the
	// scheduler the default mode cost the headline call + 0.02-0.03 ms and the 4K frame + 0.04-0.08 ms over the zero-copy
	// mode; pinned, + 0.00-0.02: profiles/r04/carrier_pinning_ab.txt).
	struct staging_frame
	{
		void* ptr = nullptr;
		size_t bytes = 0;
		bool registered = false;
		int view_device = -1;	   // the device `view` is the address on (the one that was current when it was asked for)
		void* view = nullptr;
		hipError_t reserve(size_t wanted, int numa_node); // grows (contents lost: the caller wipes); ptr all zero after a successful growth
		void release();
		~staging_frame() { release(); }
		template <typename T>
		T* as() const
		{
			return static_cast<T*>(ptr);
		}
	};

	struct frame_delivery
	{
		staging_frame frame; // uint32 per pixel; all zero between frames
		int numa_node = -1;	 // where the frame's pages should live
		bool dirty = false;	 // not all zero (a failed frame): wiped by the next begin
		pixel_carrier carrier;

		frame_delivery(unsigned helpers, int node);
		// before the launch: the frame in place and all zero, its address as the current device sees it.  The carrier's threads
		// are not told yet —
		rt_hip_status begin(uint32_t* caller_pixels, size_t pixels, uint32_t** out_device_view, bool bottom_first = true);
		// — but right BEHIND the launch: waking them (a futex call, and however long the host's scheduler takes) then runs
		// beside the kernel instead of in front of it
		void launched()
		{
			carrier.announce();
		}
		// the same frame as `device` sees it (direct frames of several GPUs); leaves that device current; NULL on failure
		uint32_t* view_on(int device);
		void finish();
		void abandon()
		{
			carrier.abandon();
			dirty = true;
		}
	};
	// the context's delivery, made on first use (NULL: out of memory)
	frame_delivery* delivery_of(rt_hip_ctx* ctx);

	// ---- frame_call.hip: the steps the single-context drop-in calls share ----
	// `who` is the entry point's name, the prefix of every message.
	// "contexts from rt_hip_create only": the refusal of a multi-GPU, rank or frame-group context
	rt_hip_status single_context_only(const char* who, const rt_hip_ctx* ctx);
	// the caller's scene checked, fingerprinted and resident on `ctx`; starts the call's phases and sets its upload_ms (the whole scene
	// check, fingerprint pass included)
	rt_hip_status resident_scene(rt_hip_ctx* ctx, const rt_hip_scene* scene, scene_request& request);
	// everything the frame's pixels depend on; `flags` masked by the caller (pass_frame_flags, history_frame_flags)
	frame_key frame_key_of(const scene_request& request, const rt_hip_scene* scene, uint32_t width, uint32_t height, uint64_t seed, uint32_t flags);
	// RT_HIP_FLAG_TRACE_BOXES for the guide kernel: does it trace the resident scene's boxes?  Refused beyond box_max_count
	rt_hip_status guide_boxes(const char* who, const rt_hip_ctx* ctx, uint32_t flags, bool* trace_boxes);
	// a call on a finished accumulation has launched nothing: its stats say so
	void nothing_launched(rt_hip_ctx* ctx);
	// Device buffers by the names the caller knows them under (NULL: not given).  An output that overlaps an input is refused as
	// "<out> overlaps <in> (<why>)"; two outputs that overlap as `among_outputs`, or by their names where that is NULL.
	struct named_buffer
	{
		const void* ptr;
		size_t bytes;
		const char* name;
	};
	rt_hip_status refuse_overlaps(const char* who, std::initializer_list<named_buffer> outputs, std::initializer_list<named_buffer> inputs, const char* why, const char* among_outputs = nullptr);

	// What one drop-in call has put on its stream, and the module-owned frame it has begun.  On EVERY exit that has not drained
	// and finished, the destructor first waits for the stream and only then abandons the frame — in that order by construction:
	// whatever the call enqueued has drained before the staging frame is abandoned (wiped, or on growth unmapped, by the next
	// begin()).  A launch can fail AFTER its kernel is enqueued (hipGetLastError, the timing events, the counters' copy): without
	// the wait the device would go on storing pixels into a frame the zero-means-pending protocol has already handed to the next
	// call — or into unmapped memory — and results would still be landing in a staging buffer the next call re-uses.  (ADVICE r4;
	// settle_members below is the same rule for several devices.)
	struct frame_scope
	{
		hipStream_t stream;
		bool armed = false;				   // the device may be storing into host memory: no return before the stream has drained
		frame_delivery* carried = nullptr; // begun and not finished: no thread keeps copying, the staging frame is wiped before its next use
		explicit frame_scope(hipStream_t s, bool arm = false) : stream(s), armed(arm) {}
		frame_scope(const frame_scope&) = delete;
		frame_scope& operator=(const frame_scope&) = delete;
		~frame_scope()
		{
			if (armed && hipStreamSynchronize(stream) != hipSuccess)
				(void)hipGetLastError();
			if (carried)
				carried->abandon();
		}
		hipError_t drain() // the success path's wait (a failed one is tried once more on the way out)
		{
			const hipError_t drained = hipStreamSynchronize(stream);
			armed = drained != hipSuccess;
			return drained;
		}
	};

	// The carried shape (rt_hip_render, rt_hip_render_progressive, rt_hip_render_adaptive): the kernels store finished pixels into the
	// module-owned page-locked frame, the carrier's threads take them on into the caller's buffer (frame.hip), and the float mean
	// lands in the module's own page-locked buffer and is copied on from there.
	//   open      the context's delivery (a finished accumulation uses its carrier alone)
	//   begin     the frame in place, the float buffers reserved, the scope armed; `direct`: the caller's own page-locked frame as
	//             the device sees it — nothing is staged (RT_HIP_FLAG_PERSISTENT_FRAME)
	//   ... the launch into d_frame / d_rgb ...
	//   launched  directly behind the launch: the carrier's threads wake beside the kernel
	//   ... whatever else the call enqueues ...
	//   deliver   the float copy, the wait on `end` (the event behind the call's device work; NULL: no stats kept) and on the stream,
	//             the rest of the frame and the float mean in the caller's memory; `e`: what the caller's own enqueues returned
	//   account   behind the caller's own bookkeeping: readback_ms, the host phases, render_ms from render_begin to `end`, the stats
	struct carried_frame
	{
		rt_hip_ctx* ctx;
		uint32_t* pixels_rgba8888;
		float* rgb_f32;
		size_t pixels;
		frame_scope scope;
		frame_delivery* delivery = nullptr;
		uint32_t* d_frame = nullptr; // where the launch stores packed pixels ...
		float* d_rgb = nullptr;		 // ... and the float mean (NULL: not asked for)
		hipEvent_t end = nullptr;
		std::chrono::steady_clock::time_point issued{}, waited_from{};
		carried_frame(rt_hip_ctx* c, uint32_t* caller_pixels, float* caller_rgb, size_t n) : ctx(c), pixels_rgba8888(caller_pixels), rgb_f32(caller_rgb), pixels(n), scope(c->stream) {}
		rt_hip_status open(const char* who);
		rt_hip_status begin(uint32_t* direct = nullptr);
		void launched()
		{
			if (scope.carried)
				scope.carried->launched();
		}
		rt_hip_status deliver(hipEvent_t end_event, hipError_t e = hipSuccess);
		rt_hip_status account(std::chrono::steady_clock::time_point entered, rt_hip_stats* stats);
	};

	// The staged shape (rt_hip_render_temporal, rt_hip_render_upscaled, rt_hip_denoise_progressive): the results lie in device buffers;
	// packed pixels, an optional float image and an optional count word go to the feature's page-locked landing, then by memcpy into
	// the caller's plain memory (the runtime never touches the caller's pages).
	struct staged_results
	{
		pinned_buffer& staging;
		size_t rgba_bytes, rgb_bytes; // rgb_bytes 0: no float image
		bool word;
		std::chrono::steady_clock::time_point waited_from{}; // where readback_ms starts
		uint32_t words = 1;									 // how many words `word` is (rt_hip_render_tonemapped: its state record)
		hipError_t reserve() { return staging.reserve(rgba_bytes + rgb_bytes + (word ? words * sizeof(uint32_t) : 0u)); }
		// enqueues the copies on the scope's stream, drains it, fills the caller's pointers; *out_word (may be NULL) is the word
		rt_hip_status deliver(frame_scope& scope, const void* d_packed, const void* d_rgb, const void* d_word, uint32_t* pixels_rgba8888, float* rgb_f32, uint32_t* out_word);
	};

	// After the first launch of a multi-GPU frame nothing may return before every member's stream has drained: a member
	// that is still storing into the frame (or into stripe buffers a later call would re-use) must not outlive the call
	// that reported the failure.  Also puts the root's device back as the current one.
	struct settle_members
	{
		rt_hip_ctx* root;
		bool armed = false;
		explicit settle_members(rt_hip_ctx* r) : root(r) {}
		settle_members(const settle_members&) = delete;
		settle_members& operator=(const settle_members&) = delete;
		~settle_members()
		{
			if (!armed)
				return;
			for (rt_hip_ctx* member : root->peers)
				if (hipSetDevice(member->device) == hipSuccess)
					(void)hipStreamSynchronize(member->stream);
			if (hipSetDevice(root->device) == hipSuccess)
				(void)hipStreamSynchronize(root->stream);
			(void)hipGetLastError();
		}
	};
}
