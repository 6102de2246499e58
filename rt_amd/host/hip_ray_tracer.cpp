// rt_amd/host/hip_ray_tracer.cpp — the MI355X renderer as an rt plug-in, against the mirror of the rt interfaces in rt_amd/host.
//
// The reference-side code the path needs is two files: shim/rt_hip_plugin.hpp, the plug-in's body (which context, the RT_HIP_*
// environment, the gather of the scene's struct-of-arrays column pointers and the camera matrix into the POD rt_hip_scene, which
// frame call of the C ABI in include/rt_hip.h a render() becomes), and shim/hip_ray_tracer.cpp, the renderer_interface subclass
// registered with REGISTER_RENDERER like every rt renderer (selectable as `--renderer hip`) against the REAL rt / muu headers
// (INTEGRATION.md).  This file is shim/hip_ray_tracer.cpp with the mirror's include block: from the marker line on the two are one
// text, so that what is built and run here (rt_headless; tests/native/plugin_calls.cpp on the CPU) is the text that ships.
#include "renderer.hpp"

#include "../../shim/rt_hip_plugin.hpp"

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
