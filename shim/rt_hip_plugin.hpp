// shim/rt_hip_plugin.hpp — the body of the hip_ray_tracer plug-in, written once.
//
// Everything the plug-in does that needs only the C ABI (rt_hip.h, found on the include path) and the standard library: which
// context to create, the RT_HIP_* environment, the emission table's upkeep, which of the module's frame calls a render() becomes and
// what it falls back to.  It names no rt, muu or mirror type; gather_scene() is a template over the scene and viewport types and uses
// only the accessor names both trees have.  Two files include it and add the renderer_interface subclass and the registrations:
//   shim/hip_ray_tracer.cpp          against the real rt / muu headers (goes into rt's src/renderers/ together with this file)
//   rt_amd/host/hip_ray_tracer.cpp   against the mirror in rt_amd/host: compiled into rt_headless, and into
//                                    tests/native/plugin_calls.cpp, which records every call this text makes (tests/test_plugin_calls.py)
//
// Behaviour at the boundary:
//   - the rt_hip context is created lazily on the first render() and destroyed with the renderer object;
//   - render() is noexcept and returns void: on any failure it prints `error: ...` to stderr (the reference's
//     style, src/main.cpp:43-47) and leaves the caller's pre-cleared frame (src/main.cpp:318) untouched;
//   - the call blocks until the frame is in `pixels`;
//   - entry points added to the C ABI after this text's other calls are declared weak and tested for null: a caller may meet an
//     older library.
#pragma once

#include <rt_hip.h>

// Additions to ABI 6 that came after this plug-in's other calls: declared WEAK here, so that a plug-in built from this text still loads
// against a librt_hip.so that lacks them, and tested for null before use (tonemap_wanted below).
extern "C"
{
	__attribute__((weak)) rt_hip_status rt_hip_render_tonemapped(rt_hip_ctx* ctx, const rt_hip_scene* scene, uint32_t* pixels_rgba8888, uint32_t width, uint32_t height, uint64_t seed, uint32_t flags, const rt_hip_tonemap_params* params,
																 float* rgb_f32, rt_hip_stats* stats, rt_hip_tonemap_info* out_info);
	__attribute__((weak)) rt_hip_status rt_hip_tonemap_from_spec(const char* spec, rt_hip_tonemap_params* out_params);
	// ... and after those (bloom_wanted below)
	__attribute__((weak)) rt_hip_status rt_hip_render_bloomed(rt_hip_ctx* ctx, const rt_hip_scene* scene, uint32_t* pixels_rgba8888, uint32_t width, uint32_t height, uint64_t seed, uint32_t flags, const rt_hip_bloom_params* bloom_params,
															  const rt_hip_tonemap_params* tonemap_params, float* rgb_f32, rt_hip_stats* stats, rt_hip_tonemap_info* out_tonemap_info);
	__attribute__((weak)) rt_hip_status rt_hip_bloom_from_spec(const char* spec, rt_hip_bloom_params* out_params);
	// ... and after those (lens_wanted below)
	__attribute__((weak)) rt_hip_status rt_hip_set_lens(rt_hip_ctx* ctx, const rt_hip_lens* lens);
	__attribute__((weak)) rt_hip_status rt_hip_lens_from_spec(const char* spec, rt_hip_lens* out_lens);
}

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <string_view>
#include <vector>

namespace rt_hip_plugin
{
	// RT_HIP_DEVICES picks the GPUs: unset = GPU 0 (or RT_HIP_DEVICE=<n>); "all" = every visible GPU; "0,1,2,3" = those, the
	// first being the root that assembles the frame.  More than one GPU = one rt_hip_create_multi context: the frame is
	// split into row stripes, gathered over RCCL and delivered by the same single blocking call.
	//
	// RT_HIP_GROUP="<shm name>:<rank>:<world>" makes this process ONE RANK of a renderer whose ranks are processes, one per
	// GPU (RT_HIP_DEVICE picks this process's): rt_hip_create + rt_hip_join_frame_group.  The image the application hands to
	// render() must then be every rank's mapping of one shared buffer (rt_headless --shared-frame); render()
	// returns on every rank when the whole frame is in it.
	inline rt_hip_status create_context(rt_hip_ctx** ctx)
	{
		const char* list = std::getenv("RT_HIP_DEVICES");
		if (const char* group = std::getenv("RT_HIP_GROUP"); group && *group)
		{
			char name[208] = {};
			int rank = -1, world = 0;
			const char* const first_colon = std::strchr(group, ':');
			if (!first_colon || static_cast<size_t>(first_colon - group) >= sizeof(name) || std::sscanf(first_colon, ":%d:%d", &rank, &world) != 2)
			{
				std::cerr << "error: hip_ray_tracer: RT_HIP_GROUP must look like /name:rank:world\n";
				return RT_HIP_INVALID_ARGUMENT;
			}
			std::memcpy(name, group, static_cast<size_t>(first_colon - group));
			const char* device = std::getenv("RT_HIP_DEVICE");
			if (const rt_hip_status st = rt_hip_create(ctx, device ? std::atoi(device) : 0))
				return st;
			if (const rt_hip_status st = rt_hip_join_frame_group(*ctx, rank, world, name, 0))
			{
				rt_hip_destroy(*ctx); // (keeps the message)
				*ctx = nullptr;
				return st;
			}
			return RT_HIP_OK;
		}
		if (!list || !*list)
		{
			const char* device = std::getenv("RT_HIP_DEVICE");
			return rt_hip_create(ctx, device ? std::atoi(device) : 0);
		}
		int devices[64];
		int n = 0;
		if (std::strcmp(list, "all") == 0)
		{
			if (rt_hip_device_count(&n) != RT_HIP_OK)
				return RT_HIP_NO_DEVICE;
			n = n > 64 ? 64 : n;
			for (int i = 0; i < n; i++)
				devices[i] = i;
		}
		else
		{
			for (const char* p = list; *p && n < 64;)
			{
				char* end = nullptr;
				const long v = std::strtol(p, &end, 10);
				if (end == p)
					break;
				devices[n++] = static_cast<int>(v);
				p = (*end == ',') ? end + 1 : end;
			}
		}
		// RT_HIP_FRAME=direct (or locked+direct): no gather — every GPU stores its pixels straight into the frame (the module's
		// own page-locked one by default; rt's own back buffer with "locked")
		const char* frame = std::getenv("RT_HIP_FRAME");
		const uint32_t flags = (frame && std::strstr(frame, "direct")) ? static_cast<uint32_t>(RT_HIP_MULTI_DIRECT_FRAME) : static_cast<uint32_t>(RT_HIP_MULTI_NONE);
		return rt_hip_create_multi(ctx, devices, n, flags); // n == 0 fails there with a message
	}

	// The default passes NO frame flag: the module renders into a page-locked frame of its own and its host threads carry the
	// pixels into rt's image while the frame is still being traced.  rt's image stays plain memory to the module — rt
	// re-creates its images on resize, also while another renderer is the active one (src/window.cpp:198-203,213), and a
	// renderer's render() is noexcept / void with nowhere to report a fault (src/renderer.hpp:11).
	// RT_HIP_FRAME=locked opts in to RT_HIP_FLAG_PERSISTENT_FRAME (rt's image itself is page-locked and mapped; the kernels
	// store straight into it, a few tens of microseconds less per frame): only for a build of rt that calls
	// rt_hip_forget_frame wherever it re-creates its images (INTEGRATION.md §3 "The back buffer").
	inline uint32_t frame_flags()
	{
		static const uint32_t flags = []
		{
			const char* frame = std::getenv("RT_HIP_FRAME");
			return (frame && std::strstr(frame, "locked")) ? static_cast<uint32_t>(RT_HIP_FLAG_PERSISTENT_FRAME) : static_cast<uint32_t>(RT_HIP_FLAG_NONE);
		}();
		return flags;
	}

	// RT_HIP_ACCEL=bvh opts in to RT_HIP_FLAG_BVH: the spheres through a bounding volume hierarchy, the same frame bit for bit
	// (for scenes of thousands of spheres; the preview ignores it)
	inline uint32_t accel_flags()
	{
		static const uint32_t flags = []
		{
			const char* accel = std::getenv("RT_HIP_ACCEL");
			// RT_HIP_TRACE_BOXES=1 opts in to RT_HIP_FLAG_TRACE_BOXES: the traced frame hits the scene's boxes too (the preview
			// draws them anyway and ignores the flag; progressive frames refuse it)
			const char* boxes = std::getenv("RT_HIP_TRACE_BOXES");
			// RT_HIP_BOX_BVH=1, next to it, opts in to RT_HIP_FLAG_BOX_BVH: the boxes through a hierarchy of their own, any number of them,
			// the same frame bit for bit (without RT_HIP_TRACE_BOXES=1 the module refuses the flag by name; so do temporal frames)
			const char* box_bvh = std::getenv("RT_HIP_BOX_BVH");
			const uint32_t trace_boxes = ((boxes && std::strcmp(boxes, "1") == 0) ? static_cast<uint32_t>(RT_HIP_FLAG_TRACE_BOXES) : static_cast<uint32_t>(RT_HIP_FLAG_NONE))
										 | ((box_bvh && std::strcmp(box_bvh, "1") == 0) ? static_cast<uint32_t>(RT_HIP_FLAG_BOX_BVH) : static_cast<uint32_t>(RT_HIP_FLAG_NONE));
			if (accel && std::strcmp(accel, "bvh-device") == 0) // ... and builds the hierarchy on the GPU (RT_HIP_FLAG_BVH_DEVICE_BUILD)
				return static_cast<uint32_t>(RT_HIP_FLAG_BVH | RT_HIP_FLAG_BVH_DEVICE_BUILD) | trace_boxes;
			return ((accel && std::strcmp(accel, "bvh") == 0) ? static_cast<uint32_t>(RT_HIP_FLAG_BVH) : static_cast<uint32_t>(RT_HIP_FLAG_NONE)) | trace_boxes;
		}();
		return flags;
	}

	// RT_HIP_PROGRESSIVE=<samples per pass> makes render() one PASS of a progressive frame (rt_hip_render_progressive): every call adds
	// that many samples per pixel to the frame in flight and shows it as it then stands, until the scene's samples_per_pixel are in —
	// a noisy frame at once that converges while the camera rests; anything the frame depends on starts it again.  0 / unset: every
	// render() is a whole frame.  (Not for the preview, which is one ray per pixel.)
	inline uint32_t progressive_pass_samples()
	{
		static const uint32_t samples = []
		{
			const char* progressive = std::getenv("RT_HIP_PROGRESSIVE");
			return progressive ? static_cast<uint32_t>(std::strtoul(progressive, nullptr, 0)) : 0u;
		}();
		return samples;
	}

	// RT_HIP_DENOISE=1, next to RT_HIP_PROGRESSIVE: the frames of an UNFINISHED accumulation — the noisy ones a user looks at while the
	// frame converges — are delivered through the guide-buffer denoiser (rt_hip_denoise_progressive, default parameters); the finished
	// frame is delivered as it is.  RT_HIP_DENOISE=always (rt_headless --denoise) filters the finished frame as well.  0 = off.
	inline uint32_t denoise_mode()
	{
		static const uint32_t mode = []
		{
			const char* denoise = std::getenv("RT_HIP_DENOISE");
			if (denoise && std::strcmp(denoise, "always") == 0)
				return 2u;
			return (denoise && std::strcmp(denoise, "1") == 0) ? 1u : 0u;
		}();
		return mode;
	}

	// RT_HIP_TEMPORAL=1 makes every render() ONE FRAME of temporal accumulation (rt_hip_render_temporal): the frame is traced whole, as
	// without the variable, and blended with the history the context keeps ACROSS camera moves — what RT_HIP_PROGRESSIVE cannot do,
	// which starts again whenever the matrix changes.  With RT_HIP_DENOISE=1 or always the blended frame also goes through the a-trous
	// filter at its defaults.  Every frame gets a seed of its own: the frame's number, or RT_HIP_SEED + the frame's number when the seed
	// is pinned — reproducible, yet no two frames trace the same samples.  Where RT_HIP_PROGRESSIVE is set it wins.  (Not for the preview.)
	inline bool temporal_frames()
	{
		static const bool on = []
		{
			const char* temporal = std::getenv("RT_HIP_TEMPORAL");
			const bool wanted = temporal && std::strcmp(temporal, "1") == 0;
			if (wanted && progressive_pass_samples())
			{
				std::cerr << "error: hip_ray_tracer: RT_HIP_TEMPORAL is ignored: RT_HIP_PROGRESSIVE is set and wins\n";
				return false;
			}
			return wanted;
		}();
		return on;
	}

	// RT_HIP_ADAPTIVE=<threshold> makes render() one PASS of an ADAPTIVE accumulation (rt_hip_render_adaptive): passes of RT_HIP_PROGRESSIVE
	// samples (16 where that is unset) over the pixels that have not converged yet, until none is left or the scene's samples_per_pixel
	// are in.  The threshold replaces the default parameters' (the other two stay; min_samples is at least two passes).  Where it is set
	// it wins over RT_HIP_PROGRESSIVE alone and over RT_HIP_TEMPORAL.  A driver that wants to know where the accumulation stands asks the
	// module (rt_hip_adaptive_last_info), as rt_headless --adaptive does.  A renderer of several GPUs refuses adaptive passes: that is said
	// once, and its frames are rt_hip_render's.  A negative or unreadable value, or none: off.  (Not for the preview.)
	inline float adaptive_threshold()
	{
		static const float threshold = []
		{
			const char* adaptive = std::getenv("RT_HIP_ADAPTIVE");
			if (!adaptive || !*adaptive)
				return -1.0f;
			char* end = nullptr;
			const float value = std::strtof(adaptive, &end);
			if (end == adaptive || *end || !(value >= 0.0f))
			{
				std::cerr << "error: hip_ray_tracer: RT_HIP_ADAPTIVE='" << adaptive << "' is not a threshold >= 0: ignored\n";
				return -1.0f;
			}
			return value;
		}();
		return threshold;
	}

	// RT_HIP_UPSCALE=K (2 .. 4; rt_headless --upscale K) makes render() ONE UPSCALED FRAME (rt_hip_render_upscaled): the frame is traced at
	// ceil(size / K) and rebuilt at full size by the guided upsampler.  With RT_HIP_DENOISE=1 or always the traced low
	// frame goes through the a-trous filter at its defaults first.  Where RT_HIP_ADAPTIVE, RT_HIP_TEMPORAL or RT_HIP_PROGRESSIVE is set, that
	// one wins; with RT_HIP_LIGHTS, or on a renderer of several GPUs, the module refuses, which is said once, and the frames are
	// rt_hip_render's.  Anything but 2, 3 or 4: off (an unreadable value is said).  (Not for the preview.)
	inline uint32_t upscale_factor()
	{
		static const uint32_t factor = []() -> uint32_t
		{
			const char* upscale = std::getenv("RT_HIP_UPSCALE");
			if (!upscale || !*upscale || std::strcmp(upscale, "0") == 0 || std::strcmp(upscale, "1") == 0)
				return 0u;
			char* end = nullptr;
			const unsigned long value = std::strtoul(upscale, &end, 10);
			if (end == upscale || *end || value < 2ul || value > 4ul)
			{
				std::cerr << "error: hip_ray_tracer: RT_HIP_UPSCALE='" << upscale << "' is not a factor of 2 .. 4: ignored\n";
				return 0u;
			}
			return static_cast<uint32_t>(value);
		}();
		return factor;
	}

	// RT_HIP_LIGHTS="KEY=R,G,B;KEY=V;..." (rt_headless --light) makes materials LIGHTS (RT_HIP_FLAG_EMISSION): rt::materials has no emission
	// column, so the table comes from this text and the scene's material names (rt_hip_lights_from_spec: a KEY is a material's name, or its
	// index) and is handed to the context (rt_hip_set_emission) — again whenever the materials change.  Unset or empty: no lights.  One-shot
	// frames only: progressive, adaptive and temporal frames refuse the flag by name.  (Not for the preview, which ignores it.)
	// RT_HIP_DIRECT_LIGHT=1 (rt_headless --direct-light) adds RT_HIP_FLAG_DIRECT_LIGHT to those frames: lambert surfaces sample the sphere lights
	// directly.  Without RT_HIP_LIGHTS it does nothing.
	inline bool direct_light_wanted()
	{
		static const bool wanted = []
		{
			const char* direct = std::getenv("RT_HIP_DIRECT_LIGHT");
			return direct && *direct && std::string_view{ direct } != "0";
		}();
		return wanted;
	}

	inline const char* lights_spec()
	{
		static const char* const spec = []
		{
			const char* lights = std::getenv("RT_HIP_LIGHTS");
			return (lights && *lights) ? lights : nullptr;
		}();
		return spec;
	}

	// RT_HIP_TONEMAP=CURVE[:EXPOSURE] (none, reinhard or aces; auto or a positive number; rt_headless --tonemap) makes a one-shot render() of
	// the two tracers ONE TONE-MAPPED FRAME (rt_hip_render_tonemapped): traced as without the variable — lights and all —
	// then exposed and mapped on the device.  It is IGNORED, which is said once, where a frame mode (RT_HIP_ADAPTIVE, RT_HIP_TEMPORAL,
	// RT_HIP_PROGRESSIVE, RT_HIP_UPSCALE) is set, for the preview, where the library lacks the call, where the text cannot be read and where
	// the module refuses (a renderer of several GPUs): the frames are rt_hip_render's then.  Unset or empty: off, and nothing is said.
	inline const char* tonemap_spec()
	{
		static const char* const spec = []
		{
			const char* tonemap = std::getenv("RT_HIP_TONEMAP");
			return (tonemap && *tonemap) ? tonemap : nullptr;
		}();
		return spec;
	}

	// RT_HIP_BLOOM=default or KEY=VALUE,... (intensity, threshold, knee, scatter, levels; rt_headless --bloom) makes a one-shot render() of the
	// two tracers ONE BLOOMED FRAME (rt_hip_render_bloomed): traced as without the variable, then the glow of what is
	// brighter than the display added on the device, then exposed and mapped with RT_HIP_TONEMAP's curve — or, without that variable, with
	// none:1, which is the plain square-root finish.  It is IGNORED, which is said once, for the reasons RT_HIP_TONEMAP is: a frame mode, the
	// preview, a library that lacks the call, a text that cannot be read, a module that refuses (a renderer of several GPUs); the frames are
	// rt_hip_render_tonemapped's then where RT_HIP_TONEMAP is on, and rt_hip_render's otherwise.  Unset or empty: off, and nothing is said.
	inline const char* bloom_spec()
	{
		static const char* const spec = []
		{
			const char* bloom = std::getenv("RT_HIP_BLOOM");
			return (bloom && *bloom) ? bloom : nullptr;
		}();
		return spec;
	}

	// RT_HIP_LENS=aperture=A,focus=F (rt_headless --lens) gives the one-shot frames of the two tracers a THIN LENS (RT_HIP_FLAG_THIN_LENS,
	// DESIGN.md §3.17): the text is read once (rt_hip_lens_from_spec), the lens handed to the context (rt_hip_set_lens) and the flag added to
	// rt_hip_render, rt_hip_render_tonemapped and rt_hip_render_bloomed.  It is IGNORED, which is said once, where a frame mode
	// (RT_HIP_ADAPTIVE, RT_HIP_TEMPORAL, RT_HIP_PROGRESSIVE, RT_HIP_UPSCALE) or RT_HIP_LIGHTS is set, where the library lacks the calls, where
	// the text cannot be read and where the module refuses the lens: the frames are the pinhole's then.  The preview ignores it without a
	// word (it is one ray through the pixel's centre).  Unset or empty: off, and nothing is said.
	inline const char* lens_spec()
	{
		static const char* const spec = []
		{
			const char* lens = std::getenv("RT_HIP_LENS");
			return (lens && *lens) ? lens : nullptr;
		}();
		return spec;
	}

	// The struct-of-arrays columns (soagen column accessors, src/soa.hpp), the two sampling scalars and the camera matrix as the POD
	// the C ABI takes: pointers are borrowed for the call.  The matrix goes element-wise through m(r, c): independent of muu's storage
	// order (accessor form: src/scene.cpp:179).  `view` is scene.camera.viewport(size of the frame) (mg_ray_tracer.cpp:180).
	template <typename Scene, typename Viewport>
	rt_hip_scene gather_scene(const Scene& scene, const Viewport& view)
	{
		static_assert(sizeof(*scene.materials.type()) == sizeof(uint32_t));	  // material_type
		static_assert(sizeof(*scene.materials.albedo()) == 4 * sizeof(float)); // rt::colour

		rt_hip_scene s{};
		s.n_spheres = static_cast<uint32_t>(scene.spheres.size());
		s.sphere_center_x = scene.spheres.center_x();
		s.sphere_center_y = scene.spheres.center_y();
		s.sphere_center_z = scene.spheres.center_z();
		s.sphere_radius = scene.spheres.radius();
		s.sphere_material = scene.spheres.material();
		s.n_planes = static_cast<uint32_t>(scene.planes.size());
		s.plane_normal_x = scene.planes.normal_x();
		s.plane_normal_y = scene.planes.normal_y();
		s.plane_normal_z = scene.planes.normal_z();
		s.plane_d = scene.planes.d();
		s.plane_material = scene.planes.material();
		s.n_materials = static_cast<uint32_t>(scene.materials.size());
		s.material_type = reinterpret_cast<const uint32_t*>(scene.materials.type());
		s.material_albedo = reinterpret_cast<const float*>(scene.materials.albedo());
		s.material_roughness = scene.materials.roughness();
		s.material_reflectivity = scene.materials.reflectivity();
		s.n_boxes = static_cast<uint32_t>(scene.boxes.size()); // drawn by the preview; traced under RT_HIP_FLAG_TRACE_BOXES only
		s.box_center_x = scene.boxes.center_x();
		s.box_center_y = scene.boxes.center_y();
		s.box_center_z = scene.boxes.center_z();
		s.box_extents_x = scene.boxes.extents_x();
		s.box_extents_y = scene.boxes.extents_y();
		s.box_extents_z = scene.boxes.extents_z();
		s.box_material = scene.boxes.material();
		s.samples_per_pixel = scene.samples_per_pixel;
		s.max_bounces = scene.max_bounces;
		for (size_t r = 0; r < 4; r++)
			for (size_t c = 0; c < 4; c++)
				s.inverse_view_projection[r * 4 + c] = view.inverse_view_projection(r, c);
		return s;
	}

	// What one renderer object keeps between frames, and its render().  `mode` is the renderer's own flag: 0 = mg_ray_tracer's scatter
	// table; RT_HIP_FLAG_SM_MATERIALS = sm_ray_tracer's (dielectrics refract); RT_HIP_FLAG_PREVIEW = the one-ray-per-pixel preview of
	// src/renderers/rasterizer.cpp, which takes none of the frame modes and no lights
	struct renderer_state
	{
		rt_hip_ctx* ctx = nullptr;
		bool failed_to_create = false;
		uint64_t frame_number = 0;
		bool temporal_unsupported = false; // RT_HIP_TEMPORAL on a renderer of several GPUs: refused once, then whole frames as without it
		bool adaptive_unsupported = false; // RT_HIP_ADAPTIVE on such a renderer: likewise
		bool upscale_unsupported = false;  // RT_HIP_UPSCALE on such a renderer, or with lights: likewise
		bool tonemap_decided = false, tonemap_on = false; // RT_HIP_TONEMAP: looked at once; on: one-shot frames are rt_hip_render_tonemapped's
		rt_hip_tonemap_params tonemap_params{};			  // ... with these, as rt_hip_tonemap_from_spec read them
		bool bloom_decided = false, bloom_on = false;	  // RT_HIP_BLOOM: looked at once; on: one-shot frames are rt_hip_render_bloomed's
		rt_hip_bloom_params bloom_params{};				  // ... with these, as rt_hip_bloom_from_spec read them
		rt_hip_tonemap_params bloom_curve{};			  // ... and this curve: RT_HIP_TONEMAP's where that is on, none:1 otherwise
		bool lens_decided = false, lens_on = false;		  // RT_HIP_LENS: looked at once; on: the context holds the lens and one-shot frames carry RT_HIP_FLAG_THIN_LENS
		std::vector<std::string> light_names; // RT_HIP_LIGHTS: the material names the context's emission table was made from
		bool lights_set = false;

		renderer_state() = default;
		renderer_state(const renderer_state&) = delete;
		renderer_state& operator=(const renderer_state&) = delete;
		~renderer_state() { rt_hip_destroy(ctx); }

		// RT_HIP_FLAG_EMISSION with the context's table made from RT_HIP_LIGHTS and these `n` material names; false: it could not be (said)
		bool light_flags(uint32_t mode, const std::string* names, size_t n, uint32_t& flags)
		{
			flags = RT_HIP_FLAG_NONE;
			const char* const spec = lights_spec();
			if (!spec || mode == RT_HIP_FLAG_PREVIEW)
				return true;
			if (!lights_set || light_names.size() != n || !std::equal(light_names.begin(), light_names.end(), names))
			{
				lights_set = false;
				light_names.assign(names, names + n);
				std::vector<const char*> c_names(n);
				for (size_t m = 0; m < n; m++)
					c_names[m] = light_names[m].c_str();
				std::vector<float> emission(n * 3u);
				if (rt_hip_lights_from_spec(spec, c_names.data(), static_cast<uint32_t>(n), emission.data()) != RT_HIP_OK
					|| rt_hip_set_emission(ctx, n ? emission.data() : nullptr, static_cast<uint32_t>(n)) != RT_HIP_OK)
				{
					std::cerr << "error: hip_ray_tracer: " << rt_hip_last_error() << "\n";
					return false;
				}
				lights_set = true;
			}
			flags = RT_HIP_FLAG_EMISSION | (direct_light_wanted() ? static_cast<uint32_t>(RT_HIP_FLAG_DIRECT_LIGHT) : static_cast<uint32_t>(RT_HIP_FLAG_NONE));
			return true;
		}

		// RT_HIP_TONEMAP, looked at once per renderer: true where its one-shot frames are to be tone-mapped; every reason why not is said here
		bool tonemap_wanted(uint32_t mode)
		{
			const char* const spec = tonemap_spec();
			if (!spec)
				return false;
			const char* const frame_mode = mode == RT_HIP_FLAG_PREVIEW	  ? nullptr
										   : adaptive_threshold() >= 0.0f ? "RT_HIP_ADAPTIVE"
										   : temporal_frames()			  ? "RT_HIP_TEMPORAL"
										   : progressive_pass_samples()	  ? "RT_HIP_PROGRESSIVE"
										   : upscale_factor()			  ? "RT_HIP_UPSCALE"
																		  : nullptr;
			if (mode == RT_HIP_FLAG_PREVIEW)
				std::cerr << "error: hip_ray_tracer: RT_HIP_TONEMAP is ignored: the preview has no float frame to map\n";
			else if (frame_mode)
				std::cerr << "error: hip_ray_tracer: RT_HIP_TONEMAP is ignored: " << frame_mode << " is set, and only one-shot frames are tone-mapped\n";
			else if (!rt_hip_render_tonemapped || !rt_hip_tonemap_from_spec)
				std::cerr << "error: hip_ray_tracer: RT_HIP_TONEMAP is ignored: this librt_hip.so has no rt_hip_render_tonemapped\n";
			else if (rt_hip_tonemap_from_spec(spec, &tonemap_params) != RT_HIP_OK)
				std::cerr << "error: hip_ray_tracer: " << rt_hip_last_error() << ": RT_HIP_TONEMAP is ignored\n";
			else
				return true;
			return false;
		}

		// RT_HIP_BLOOM, looked at once per renderer AFTER RT_HIP_TONEMAP was: true where its one-shot frames are to be bloomed; every reason why
		// not is said here
		bool bloom_wanted(uint32_t mode)
		{
			const char* const spec = bloom_spec();
			if (!spec)
				return false;
			const char* const frame_mode = mode == RT_HIP_FLAG_PREVIEW	  ? nullptr
										   : adaptive_threshold() >= 0.0f ? "RT_HIP_ADAPTIVE"
										   : temporal_frames()			  ? "RT_HIP_TEMPORAL"
										   : progressive_pass_samples()	  ? "RT_HIP_PROGRESSIVE"
										   : upscale_factor()			  ? "RT_HIP_UPSCALE"
																		  : nullptr;
			if (mode == RT_HIP_FLAG_PREVIEW)
				std::cerr << "error: hip_ray_tracer: RT_HIP_BLOOM is ignored: the preview has no float frame to bloom\n";
			else if (frame_mode)
				std::cerr << "error: hip_ray_tracer: RT_HIP_BLOOM is ignored: " << frame_mode << " is set, and only one-shot frames are bloomed\n";
			else if (!rt_hip_render_bloomed || !rt_hip_bloom_from_spec || !rt_hip_tonemap_from_spec)
				std::cerr << "error: hip_ray_tracer: RT_HIP_BLOOM is ignored: this librt_hip.so has no rt_hip_render_bloomed\n";
			else if (rt_hip_bloom_from_spec(spec, &bloom_params) != RT_HIP_OK)
				std::cerr << "error: hip_ray_tracer: " << rt_hip_last_error() << ": RT_HIP_BLOOM is ignored\n";
			else if (tonemap_on)
			{
				bloom_curve = tonemap_params;
				return true;
			}
			else if (rt_hip_tonemap_from_spec("none:1", &bloom_curve) != RT_HIP_OK) // (RT_HIP_TONEMAP unset, or ignored and said: the plain finish)
				std::cerr << "error: hip_ray_tracer: " << rt_hip_last_error() << ": RT_HIP_BLOOM is ignored\n";
			else
				return true;
			return false;
		}

		// RT_HIP_LENS, looked at once per renderer (the context exists): true where its one-shot frames carry the lens, which the context then
		// holds; every reason why not is said here
		bool lens_wanted(uint32_t mode)
		{
			const char* const spec = lens_spec();
			if (!spec || mode == RT_HIP_FLAG_PREVIEW)
				return false;
			const char* const other = adaptive_threshold() >= 0.0f ? "RT_HIP_ADAPTIVE"
									  : temporal_frames()		   ? "RT_HIP_TEMPORAL"
									  : progressive_pass_samples() ? "RT_HIP_PROGRESSIVE"
									  : upscale_factor()		   ? "RT_HIP_UPSCALE"
									  : lights_spec()			   ? "RT_HIP_LIGHTS"
																   : nullptr;
			rt_hip_lens lens{};
			if (other)
				std::cerr << "error: hip_ray_tracer: RT_HIP_LENS is ignored: " << other << " is set, and only one-shot frames without lights are taken through a lens\n";
			else if (!rt_hip_set_lens || !rt_hip_lens_from_spec)
				std::cerr << "error: hip_ray_tracer: RT_HIP_LENS is ignored: this librt_hip.so has no rt_hip_set_lens\n";
			else if (rt_hip_lens_from_spec(spec, &lens) != RT_HIP_OK || rt_hip_set_lens(ctx, &lens) != RT_HIP_OK)
				std::cerr << "error: hip_ray_tracer: " << rt_hip_last_error() << ": RT_HIP_LENS is ignored\n";
			else
				return true;
			return false;
		}

		// one frame of `s` into `pixels` (width x height, never null); `names`: the scene's n_materials material names
		void render(uint32_t mode, const rt_hip_scene& s, const std::string* names, size_t n_names, uint32_t* pixels, uint32_t width, uint32_t height) noexcept
		{
			if (failed_to_create)
				return;
			if (!ctx && create_context(&ctx) != RT_HIP_OK)
			{
				if (rt_hip_last_error()[0])
					std::cerr << "error: hip_ray_tracer: " << rt_hip_last_error() << "\n";
				failed_to_create = true;
				return;
			}

			// The reference draws fresh random numbers every frame (random_device-seeded engines, src/random.cpp:12-13): a new seed per
			// frame keeps that behaviour; RT_HIP_SEED pins it for reproducible output.
			const char* fixed = std::getenv("RT_HIP_SEED");
			const uint64_t seed = fixed ? std::strtoull(fixed, nullptr, 0) : ++frame_number;

			if (!tonemap_decided)
			{
				tonemap_decided = true;
				tonemap_on = tonemap_wanted(mode);
			}
			if (!bloom_decided)
			{
				bloom_decided = true;
				bloom_on = bloom_wanted(mode);
			}

			if (!lens_decided)
			{
				lens_decided = true;
				lens_on = lens_wanted(mode);
			}

			uint32_t lights = RT_HIP_FLAG_NONE; // (RT_HIP_LIGHTS: RT_HIP_FLAG_EMISSION, the table in place)
			if (!light_flags(mode, names, n_names, lights))
				return;
			// (RT_HIP_LENS: one-shot frames only — lens_wanted has said no wherever a frame mode or lights are set — and the preview drops it)
			const uint32_t lens = lens_on ? static_cast<uint32_t>(RT_HIP_FLAG_THIN_LENS) : static_cast<uint32_t>(RT_HIP_FLAG_NONE);

			if (mode != RT_HIP_FLAG_PREVIEW)
				if (const float threshold = adaptive_threshold(); threshold >= 0.0f && !adaptive_unsupported)
				{
					// (a seed per frame would start the accumulation again on every call: RT_HIP_SEED, or 1, for all of them)
					const uint32_t pass_samples = progressive_pass_samples() ? progressive_pass_samples() : 16u;
					rt_hip_adaptive_params params{};
					if (rt_hip_adaptive_default_params(&params) == RT_HIP_OK)
					{
						params.threshold = threshold;
						const uint64_t two_passes = 2u * ((static_cast<uint64_t>(pass_samples) + 15u) / 16u * 16u);
						if (params.min_samples < two_passes && two_passes <= 0xFFFFFFFFull)
							params.min_samples = static_cast<uint32_t>(two_passes);
					}
					const rt_hip_status st = rt_hip_render_adaptive(ctx, &s, pixels, width, height, fixed ? seed : 1u, accel_flags() | lights | mode, pass_samples, &params, nullptr, nullptr, nullptr, nullptr);
					if (st == RT_HIP_OK)
						return;
					if (st != RT_HIP_UNSUPPORTED)
					{
						std::cerr << "error: hip_ray_tracer: " << rt_hip_last_error() << "\n";
						return;
					}
					// a multi-GPU or frame-group renderer (or a flag adaptive passes do not take): said once, and from here on every frame is rt_hip_render's (below)
					std::cerr << "error: hip_ray_tracer: " << rt_hip_last_error() << ": RT_HIP_ADAPTIVE is ignored for this renderer\n";
					adaptive_unsupported = true;
				}
			if (mode != RT_HIP_FLAG_PREVIEW)
				if (temporal_frames())
				{
					const uint64_t frame_seed = fixed ? std::strtoull(fixed, nullptr, 0) + ++frame_number : seed; // (unpinned: `seed` is ++frame_number already)
					rt_hip_denoise_params filter{};
					const bool filtered = denoise_mode() != 0u && rt_hip_denoise_default_params(&filter) == RT_HIP_OK;
					const rt_hip_status st = temporal_unsupported ? RT_HIP_UNSUPPORTED : rt_hip_render_temporal(ctx, &s, pixels, width, height, frame_seed, accel_flags() | lights | mode, nullptr, filtered ? &filter : nullptr, nullptr, nullptr, nullptr);
					if (st == RT_HIP_OK)
						return;
					if (st != RT_HIP_UNSUPPORTED)
					{
						std::cerr << "error: hip_ray_tracer: " << rt_hip_last_error() << "\n";
						return;
					}
					// a multi-GPU or frame-group renderer: said once, and from here on every frame is rt_hip_render's (below), with the seed this frame got
					if (!temporal_unsupported)
						std::cerr << "error: hip_ray_tracer: " << rt_hip_last_error() << ": RT_HIP_TEMPORAL is ignored for this renderer\n";
					temporal_unsupported = true;
					if (rt_hip_render(ctx, &s, pixels, width, height, frame_seed, frame_flags() | accel_flags() | lights | mode, nullptr, nullptr) != RT_HIP_OK)
						std::cerr << "error: hip_ray_tracer: " << rt_hip_last_error() << "\n";
					return;
				}
			if (mode != RT_HIP_FLAG_PREVIEW)
				if (const uint32_t pass_samples = progressive_pass_samples())
				{
					// (a seed per frame would start the accumulation again on every call: RT_HIP_SEED, or 1, for all of them)
					rt_hip_progress progress{};
					if (rt_hip_render_progressive(ctx, &s, pixels, width, height, fixed ? seed : 1u, accel_flags() | lights | mode, pass_samples, nullptr, nullptr, &progress) != RT_HIP_OK)
						std::cerr << "error: hip_ray_tracer: " << rt_hip_last_error() << "\n";
					else if (const uint32_t denoise = denoise_mode(); denoise == 2u || (denoise == 1u && progress.samples_done < progress.samples_total))
						if (rt_hip_denoise_progressive(ctx, nullptr, pixels, nullptr, nullptr) != RT_HIP_OK) // (on failure the pass's own frame stays)
							std::cerr << "error: hip_ray_tracer: " << rt_hip_last_error() << "\n";
					return;
				}
			if (mode != RT_HIP_FLAG_PREVIEW)
				if (const uint32_t factor = upscale_factor(); factor && !upscale_unsupported)
				{
					rt_hip_denoise_params filter{};
					const bool filtered = denoise_mode() != 0u && rt_hip_denoise_default_params(&filter) == RT_HIP_OK;
					const rt_hip_status st = rt_hip_render_upscaled(ctx, &s, pixels, width, height, seed, accel_flags() | lights | mode, factor, nullptr, filtered ? &filter : nullptr, nullptr, nullptr, nullptr);
					if (st == RT_HIP_OK)
						return;
					if (st != RT_HIP_UNSUPPORTED)
					{
						std::cerr << "error: hip_ray_tracer: " << rt_hip_last_error() << "\n";
						return;
					}
					// a multi-GPU or frame-group renderer, or a flag upscaled frames do not take: said once, and from here on every frame is rt_hip_render's (below)
					std::cerr << "error: hip_ray_tracer: " << rt_hip_last_error() << ": RT_HIP_UPSCALE is ignored for this renderer\n";
					upscale_unsupported = true;
				}
			if (bloom_on) // (one-shot frames of the two tracers only: bloom_wanted; no frame flag: the pixels come from a device buffer)
			{
				const rt_hip_status st = rt_hip_render_bloomed(ctx, &s, pixels, width, height, seed, accel_flags() | lights | lens | mode, &bloom_params, &bloom_curve, nullptr, nullptr, nullptr);
				if (st == RT_HIP_OK)
					return;
				if (st != RT_HIP_UNSUPPORTED)
				{
					std::cerr << "error: hip_ray_tracer: " << rt_hip_last_error() << "\n";
					return;
				}
				// a multi-GPU or frame-group renderer: said once, and from here on every frame is the tone-mapped or the plain one (below)
				std::cerr << "error: hip_ray_tracer: " << rt_hip_last_error() << ": RT_HIP_BLOOM is ignored for this renderer\n";
				bloom_on = false;
			}
			if (tonemap_on) // (one-shot frames of the two tracers only: tonemap_wanted; no frame flag: the pixels come from a device buffer)
			{
				const rt_hip_status st = rt_hip_render_tonemapped(ctx, &s, pixels, width, height, seed, accel_flags() | lights | lens | mode, &tonemap_params, nullptr, nullptr, nullptr);
				if (st == RT_HIP_OK)
					return;
				if (st != RT_HIP_UNSUPPORTED)
				{
					std::cerr << "error: hip_ray_tracer: " << rt_hip_last_error() << "\n";
					return;
				}
				// a multi-GPU or frame-group renderer: said once, and from here on every frame is rt_hip_render's (below)
				std::cerr << "error: hip_ray_tracer: " << rt_hip_last_error() << ": RT_HIP_TONEMAP is ignored for this renderer\n";
				tonemap_on = false;
			}
			if (rt_hip_render(ctx, &s, pixels, width, height, seed, frame_flags() | accel_flags() | lights | lens | mode, nullptr, nullptr) != RT_HIP_OK)
				std::cerr << "error: hip_ray_tracer: " << rt_hip_last_error() << "\n";
		}
	};
}
