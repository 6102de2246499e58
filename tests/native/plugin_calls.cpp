// tests/native/plugin_calls.cpp — what the hip_ray_tracer plug-in asks of the module, recorded on the CPU.
//
// A stand-alone program: the mirror plug-in (rt_amd/host/hip_ray_tracer.cpp), the scene loader and, in place of librt_hip.so, a FAKE
// of the sixteen C entry points the plug-in links.  Every fake prints one line per call to stdout with each argument that is a
// decision of the plug-in; nothing here touches a GPU.  tests/test_plugin_calls.py builds it with g++ alone, runs one process per
// environment (the plug-in's getters are per-process statics) and holds the output to tests/golden/plugin_calls.txt.
//
//   plugin_calls RENDERER FRAMES [--spp N] [--rename]
// loads scenes/basic.toml, creates RENDERER through the registry and renders FRAMES frames of 8 x 4 pixels.  --spp overrides the
// scene's samples_per_pixel; --rename gives material 1 another name before the last frame (the emission table is made again).
// The plug-in's stderr is echoed after the call log.
//
// The fake is scripted by this program's own variables (comma-separated call names without the rt_hip_ prefix):
//   PLUGIN_CALLS_UNSUPPORTED   the calls that answer RT_HIP_UNSUPPORTED        e.g. render_adaptive,render_temporal
//   PLUGIN_CALLS_FAIL          the calls that answer RT_HIP_RUNTIME_ERROR      e.g. render_progressive,set_emission
//   PLUGIN_CALLS_CREATE_FAILS  set: rt_hip_create answers RT_HIP_NO_DEVICE
//   PLUGIN_CALLS_DEVICE_COUNT  what rt_hip_device_count reports (1 if unset)
// rt_hip_render_progressive reports samples_done growing by pass_samples up to the scene's samples_per_pixel.
#include "renderer.hpp"
#include <rt_hip.h>

#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <string_view>

struct rt_hip_ctx
{
	uint32_t samples_done = 0; // of the fake progressive accumulation
};

namespace
{
	std::string last_error;

	bool listed(const char* variable, std::string_view call)
	{
		const char* const list = std::getenv(variable);
		if (!list)
			return false;
		for (std::string_view rest = list; !rest.empty();)
		{
			const size_t comma = rest.find(',');
			if (rest.substr(0, comma) == call)
				return true;
			rest = comma == std::string_view::npos ? std::string_view{} : rest.substr(comma + 1);
		}
		return false;
	}

	// the scripted answer of one call, printed behind its arguments
	rt_hip_status answer(std::string_view call)
	{
		rt_hip_status st = RT_HIP_OK;
		if (listed("PLUGIN_CALLS_UNSUPPORTED", call))
			st = RT_HIP_UNSUPPORTED;
		else if (listed("PLUGIN_CALLS_FAIL", call))
			st = RT_HIP_RUNTIME_ERROR;
		if (st != RT_HIP_OK)
			last_error = "fake rt_hip_" + std::string{ call } + (st == RT_HIP_UNSUPPORTED ? " is unsupported" : " failed");
		std::printf(" -> %d\n", static_cast<int>(st));
		return st;
	}

	const char* null_or_set(const void* p) { return p ? "set" : "null"; }

	uint64_t fnv(uint64_t h, const void* data, size_t bytes)
	{
		const unsigned char* const p = static_cast<const unsigned char*>(data);
		for (size_t i = 0; i < bytes; i++)
			h = (h ^ p[i]) * 0x100000001B3ull;
		return h;
	}

	float camera_matrix[16]; // what the camera of main()'s scene gives for the frame's size, element [r * 4 + c] = m(r, c)

	// the counts, the sampling, one hash over every column's rows (a column wired to the wrong pointer changes it), and whether the
	// matrix is the camera's (said, not hashed: its last bits are the C library's)
	void print_frame(const rt_hip_ctx* ctx, const rt_hip_scene* s, const uint32_t* pixels, uint32_t width, uint32_t height)
	{
		std::printf(" ctx=%s", null_or_set(ctx));
		if (!s)
			std::printf(" scene=null");
		else
		{
			uint64_t h = 0xCBF29CE484222325ull;
			for (const float* column : { s->sphere_center_x, s->sphere_center_y, s->sphere_center_z, s->sphere_radius })
				h = fnv(h, column, s->n_spheres * sizeof(float));
			h = fnv(h, s->sphere_material, s->n_spheres * sizeof(uint32_t));
			for (const float* column : { s->plane_normal_x, s->plane_normal_y, s->plane_normal_z, s->plane_d })
				h = fnv(h, column, s->n_planes * sizeof(float));
			h = fnv(h, s->plane_material, s->n_planes * sizeof(uint32_t));
			h = fnv(h, s->material_type, s->n_materials * sizeof(uint32_t));
			h = fnv(h, s->material_albedo, s->n_materials * 4u * sizeof(float));
			h = fnv(h, s->material_roughness, s->n_materials * sizeof(float));
			h = fnv(h, s->material_reflectivity, s->n_materials * sizeof(float));
			for (const float* column : { s->box_center_x, s->box_center_y, s->box_center_z, s->box_extents_x, s->box_extents_y, s->box_extents_z })
				h = fnv(h, column, s->n_boxes * sizeof(float));
			h = fnv(h, s->box_material, s->n_boxes * sizeof(uint32_t));
			const char* const matrix = std::memcmp(s->inverse_view_projection, camera_matrix, sizeof(camera_matrix)) == 0 ? "camera's" : "WRONG";
			std::printf(" scene=spheres:%u,planes:%u,materials:%u,boxes:%u,spp:%u,bounces:%u,columns:%016" PRIx64 ",matrix:%s", s->n_spheres, s->n_planes, s->n_materials, s->n_boxes, s->samples_per_pixel, s->max_bounces, h, matrix);
		}
		std::printf(" pixels=%s %ux%u", null_or_set(pixels), width, height);
	}

	void print_filter(const char* what, const rt_hip_denoise_params* filter)
	{
		if (filter)
			std::printf(" %s=iterations:%u,squarings:%u", what, filter->iterations, filter->normal_squarings);
		else
			std::printf(" %s=null", what);
	}
}

extern "C"
{
	const char* rt_hip_last_error(void) { return last_error.c_str(); }

	rt_hip_status rt_hip_device_count(int* count)
	{
		const char* const fixed = std::getenv("PLUGIN_CALLS_DEVICE_COUNT");
		*count = fixed ? std::atoi(fixed) : 1;
		std::printf("rt_hip_device_count = %d", *count);
		return answer("device_count");
	}

	rt_hip_status rt_hip_create(rt_hip_ctx** out_ctx, int device)
	{
		std::printf("rt_hip_create device=%d", device);
		if (std::getenv("PLUGIN_CALLS_CREATE_FAILS"))
		{
			last_error = "fake rt_hip_create failed";
			std::printf(" -> %d\n", static_cast<int>(RT_HIP_NO_DEVICE));
			return RT_HIP_NO_DEVICE;
		}
		std::printf(" -> %d\n", static_cast<int>(RT_HIP_OK));
		*out_ctx = new rt_hip_ctx{};
		return RT_HIP_OK;
	}

	rt_hip_status rt_hip_create_multi(rt_hip_ctx** out_ctx, const int* devices, int n_devices, uint32_t multi_flags)
	{
		std::printf("rt_hip_create_multi devices=[");
		for (int i = 0; i < n_devices; i++)
			std::printf("%s%d", i ? "," : "", devices[i]);
		std::printf("] multi_flags=0x%x", multi_flags);
		if (n_devices <= 0) // (as the module does)
		{
			last_error = "fake rt_hip_create_multi: no devices";
			std::printf(" -> %d\n", static_cast<int>(RT_HIP_INVALID_ARGUMENT));
			return RT_HIP_INVALID_ARGUMENT;
		}
		const rt_hip_status st = answer("create_multi");
		if (st == RT_HIP_OK)
			*out_ctx = new rt_hip_ctx{};
		return st;
	}

	rt_hip_status rt_hip_join_frame_group(rt_hip_ctx* ctx, int rank, int world, const char* name, uint32_t timeout_ms)
	{
		std::printf("rt_hip_join_frame_group ctx=%s rank=%d world=%d name='%s' timeout_ms=%u", null_or_set(ctx), rank, world, name, timeout_ms);
		return answer("join_frame_group");
	}

	void rt_hip_destroy(rt_hip_ctx* ctx)
	{
		std::printf("rt_hip_destroy ctx=%s\n", null_or_set(ctx));
		delete ctx;
	}

	rt_hip_status rt_hip_render(rt_hip_ctx* ctx, const rt_hip_scene* scene, uint32_t* pixels, uint32_t width, uint32_t height, uint64_t seed, uint32_t flags, float* rgb_f32, rt_hip_stats* stats)
	{
		std::printf("rt_hip_render");
		print_frame(ctx, scene, pixels, width, height);
		std::printf(" seed=%" PRIu64 " flags=0x%x rgb_f32=%s stats=%s", seed, flags, null_or_set(rgb_f32), null_or_set(stats));
		return answer("render");
	}

	rt_hip_status rt_hip_render_progressive(rt_hip_ctx* ctx, const rt_hip_scene* scene, uint32_t* pixels, uint32_t width, uint32_t height, uint64_t seed, uint32_t flags, uint32_t pass_samples, float* rgb_f32, rt_hip_stats* stats, rt_hip_progress* out_progress)
	{
		std::printf("rt_hip_render_progressive");
		print_frame(ctx, scene, pixels, width, height);
		std::printf(" seed=%" PRIu64 " flags=0x%x pass_samples=%u rgb_f32=%s stats=%s out_progress=%s", seed, flags, pass_samples, null_or_set(rgb_f32), null_or_set(stats), null_or_set(out_progress));
		const rt_hip_status st = answer("render_progressive");
		if (st == RT_HIP_OK && ctx && scene)
		{
			const uint64_t done = static_cast<uint64_t>(ctx->samples_done) + pass_samples;
			ctx->samples_done = done < scene->samples_per_pixel ? static_cast<uint32_t>(done) : scene->samples_per_pixel;
			if (out_progress)
				*out_progress = rt_hip_progress{ ctx->samples_done, scene->samples_per_pixel, 0u, 0u };
		}
		return st;
	}

	rt_hip_status rt_hip_denoise_progressive(rt_hip_ctx* ctx, const rt_hip_denoise_params* params, uint32_t* pixels, float* rgb_f32, float* render_ms)
	{
		std::printf("rt_hip_denoise_progressive ctx=%s", null_or_set(ctx));
		print_filter("params", params);
		std::printf(" pixels=%s rgb_f32=%s render_ms=%s", null_or_set(pixels), null_or_set(rgb_f32), null_or_set(render_ms));
		return answer("denoise_progressive");
	}

	rt_hip_status rt_hip_render_temporal(rt_hip_ctx* ctx, const rt_hip_scene* scene, uint32_t* pixels, uint32_t width, uint32_t height, uint64_t seed, uint32_t flags, const rt_hip_temporal_params* temporal, const rt_hip_denoise_params* filter, float* rgb_f32, rt_hip_stats* stats, rt_hip_temporal_info* out_info)
	{
		std::printf("rt_hip_render_temporal");
		print_frame(ctx, scene, pixels, width, height);
		std::printf(" seed=%" PRIu64 " flags=0x%x temporal=%s", seed, flags, null_or_set(temporal));
		print_filter("filter", filter);
		std::printf(" rgb_f32=%s stats=%s out_info=%s", null_or_set(rgb_f32), null_or_set(stats), null_or_set(out_info));
		return answer("render_temporal");
	}

	rt_hip_status rt_hip_render_adaptive(rt_hip_ctx* ctx, const rt_hip_scene* scene, uint32_t* pixels, uint32_t width, uint32_t height, uint64_t seed, uint32_t flags, uint32_t pass_samples, const rt_hip_adaptive_params* params, float* rgb_f32, uint32_t* sample_counts, rt_hip_stats* stats, rt_hip_adaptive_info* out_info)
	{
		std::printf("rt_hip_render_adaptive");
		print_frame(ctx, scene, pixels, width, height);
		std::printf(" seed=%" PRIu64 " flags=0x%x pass_samples=%u", seed, flags, pass_samples);
		if (params)
			std::printf(" params=threshold:%.9g,floor:%.9g,min_samples:%u", static_cast<double>(params->threshold), static_cast<double>(params->floor), params->min_samples);
		else
			std::printf(" params=null");
		std::printf(" rgb_f32=%s sample_counts=%s stats=%s out_info=%s", null_or_set(rgb_f32), null_or_set(sample_counts), null_or_set(stats), null_or_set(out_info));
		return answer("render_adaptive");
	}

	rt_hip_status rt_hip_render_upscaled(rt_hip_ctx* ctx, const rt_hip_scene* scene, uint32_t* pixels, uint32_t width, uint32_t height, uint64_t seed, uint32_t flags, uint32_t factor, const rt_hip_upsample_params* upsample, const rt_hip_denoise_params* filter, float* rgb_f32, rt_hip_stats* stats, rt_hip_upscale_info* out_info)
	{
		std::printf("rt_hip_render_upscaled");
		print_frame(ctx, scene, pixels, width, height);
		std::printf(" seed=%" PRIu64 " flags=0x%x factor=%u upsample=%s", seed, flags, factor, null_or_set(upsample));
		print_filter("filter", filter);
		std::printf(" rgb_f32=%s stats=%s out_info=%s", null_or_set(rgb_f32), null_or_set(stats), null_or_set(out_info));
		return answer("render_upscaled");
	}

	// the module's defaults (include/rt_hip.h): what the plug-in changes in them is its decision, and shows in the frame call's line
	rt_hip_status rt_hip_adaptive_default_params(rt_hip_adaptive_params* out_params)
	{
		std::printf("rt_hip_adaptive_default_params");
		const rt_hip_status st = answer("adaptive_default_params");
		if (st == RT_HIP_OK)
			*out_params = rt_hip_adaptive_params{ 0.03f, 0.01f, 32u };
		return st;
	}

	rt_hip_status rt_hip_denoise_default_params(rt_hip_denoise_params* out_params)
	{
		std::printf("rt_hip_denoise_default_params");
		const rt_hip_status st = answer("denoise_default_params");
		if (st == RT_HIP_OK)
			*out_params = rt_hip_denoise_params{ 1u, 3u, 0.2f, 0.1f, 0.02f };
		return st;
	}

	rt_hip_status rt_hip_lights_from_spec(const char* spec, const char* const* material_names, uint32_t n_materials, float* out_emission_rgb)
	{
		std::printf("rt_hip_lights_from_spec spec='%s' names=[", spec ? spec : "(null)");
		for (uint32_t m = 0; m < n_materials; m++)
			std::printf("%s'%s'", m ? "," : "", material_names ? material_names[m] : "(null)");
		std::printf("] out=%s", null_or_set(out_emission_rgb));
		const rt_hip_status st = answer("lights_from_spec");
		if (st == RT_HIP_OK && out_emission_rgb)
			for (uint32_t i = 0; i < n_materials * 3u; i++)
				out_emission_rgb[i] = 1.0f;
		return st;
	}

	rt_hip_status rt_hip_set_emission(rt_hip_ctx* ctx, const float* emission_rgb, uint32_t n_materials)
	{
		std::printf("rt_hip_set_emission ctx=%s emission=%s n_materials=%u", null_or_set(ctx), null_or_set(emission_rgb), n_materials);
		return answer("set_emission");
	}
}

int main(int argc, char** argv)
{
	if (argc < 3)
	{
		std::fprintf(stderr, "usage: plugin_calls RENDERER FRAMES [--spp N] [--rename]\n");
		return 2;
	}
	const unsigned frames = static_cast<unsigned>(std::strtoul(argv[2], nullptr, 10));
	unsigned spp = 0;
	bool rename = false;
	for (int i = 3; i < argc; i++)
	{
		if (std::strcmp(argv[i], "--spp") == 0 && i + 1 < argc)
			spp = static_cast<unsigned>(std::strtoul(argv[++i], nullptr, 10));
		else if (std::strcmp(argv[i], "--rename") == 0)
			rename = true;
		else
		{
			std::fprintf(stderr, "plugin_calls: unknown argument '%s'\n", argv[i]);
			return 2;
		}
	}

	const rt::renderers::description* const desc = rt::renderers::find_by_name(argv[1]);
	if (!desc)
	{
		std::fprintf(stderr, "plugin_calls: no renderer named '%s'\n", argv[1]);
		return 2;
	}
	rt::scene scene;
	try
	{
		scene = rt::scene::load("scenes/basic.toml");
	}
	catch (const std::exception& e)
	{
		std::fprintf(stderr, "plugin_calls: %s\n", e.what());
		return 2;
	}
	if (spp)
		scene.samples_per_pixel = spp;

	// the plug-in speaks through std::cerr alone: its text is kept and echoed after the call log
	std::ostringstream said;
	std::streambuf* const terminal = std::cerr.rdbuf(said.rdbuf());
	{
		std::unique_ptr<rt::renderer_interface> renderer{ desc->create() };
		rt::image frame{ rt::vec2u{ 8u, 4u } };
		rt::image_view pixels{ frame };
		const rt::viewport view = scene.camera.viewport(pixels.size());
		for (size_t r = 0; r < 4; r++)
			for (size_t c = 0; c < 4; c++)
				camera_matrix[r * 4 + c] = view.inverse_view_projection(r, c);
		muu::thread_pool threads;
		for (unsigned f = 0; f < frames; f++)
		{
			if (rename && f + 1 == frames)
			{
				// (rt::materials hands out no mutable name: the table is made again, material 1 under another name)
				rt::materials renamed;
				for (size_t m = 0; m < scene.materials.size(); m++)
					renamed.push_back(m == 1 ? std::string{ "lamp" } : scene.materials.name()[m], scene.materials.type()[m], scene.materials.albedo()[m], scene.materials.roughness()[m], scene.materials.reflectivity()[m]);
				scene.materials = std::move(renamed);
			}
			std::printf("frame %u\n", f);
			pixels.clear(0x000000FFu);
			renderer->render(scene, pixels, threads);
		}
	}
	std::cerr.rdbuf(terminal);
	std::printf("stderr:\n%s", said.str().c_str());
	return 0;
}
