// shim/hip_ray_tracer.cpp — the reference-side binding of the MI355X renderer module.
//
// Drop this file AND shim/rt_hip_plugin.hpp (the plug-in's body: plain C ABI and standard library, no rt / muu name) into
// marzer/rt's src/renderers/, add this file to src/renderers/meson.build next to mg_ray_tracer.cpp (reference
// src/renderers/meson.build:7-12), put include/rt_hip.h on the include path and link librt_hip.so.
// This file is the only code that sees rt / muu types; everything below it is plain C.
//
// It cannot be compiled in this repository: rt's headers pull in marzer/muu, which is a network-fetched meson wrap
// (reference subprojects/muu.wrap).  That concerns the include block below and nothing else: from the marker line on
// this file is, byte for byte, rt_amd/host/hip_ray_tracer.cpp, which is compiled against a mirror of the rt interfaces
// and run by rt_headless and tests/native/plugin_calls.cpp (tests/test_plugin_calls.py holds the two files together).
//
// Replaces: mg_ray_tracer::render (reference src/renderers/mg_ray_tracer.cpp:178-205) behind
// renderer_interface::render (reference src/renderer.hpp:9-14).
#include "../scene.hpp"
#include "../image.hpp"
#include "../renderer.hpp"
MUU_DISABLE_WARNINGS;
#include <muu/thread_pool.h>
#include "rt_hip_plugin.hpp"
MUU_ENABLE_WARNINGS;

// ---- from here on shim/hip_ray_tracer.cpp and rt_amd/host/hip_ray_tracer.cpp are one text (tests/test_plugin_calls.py) ----
using namespace rt;

namespace
{
	// ModeFlags: 0 = mg_ray_tracer's scatter table; RT_HIP_FLAG_SM_MATERIALS = sm_ray_tracer's (dielectrics refract);
	// RT_HIP_FLAG_PREVIEW = the one-ray-per-pixel preview of src/renderers/rasterizer.cpp
	template <uint32_t ModeFlags>
	struct hip_renderer : renderer_interface
	{
		rt_hip_plugin::renderer_state state; // the context, destroyed with the renderer object, and what it keeps between frames

		// the passed thread pool is ignored; the call blocks until the frame is in `pixels`
		void render(const rt::scene& scene, image_view& pixels, muu::thread_pool& /*threads*/) noexcept override
		{
			if (!pixels)
				return;
			const rt_hip_scene s = rt_hip_plugin::gather_scene(scene, scene.camera.viewport(pixels.size()));
			state.render(ModeFlags, s, scene.materials.name(), scene.materials.size(), pixels.data(), pixels.size().x, pixels.size().y);
		}
	};

	struct hip_ray_tracer final : hip_renderer<RT_HIP_FLAG_NONE>
	{};
	struct hip_sm_ray_tracer final : hip_renderer<RT_HIP_FLAG_SM_MATERIALS>
	{};
	struct hip_rasterizer final : hip_renderer<RT_HIP_FLAG_PREVIEW> // could stand in for "rasterizer" at src/main.cpp:106
	{};

	REGISTER_RENDERER(hip_ray_tracer); // (first: `--renderer hip` keeps selecting the path tracer)
	REGISTER_RENDERER(hip_sm_ray_tracer);
	REGISTER_RENDERER(hip_rasterizer);
}
