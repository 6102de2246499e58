// tests/native/plugin_tonemap_fake.cpp — recording fakes of the two entry points shim/rt_hip_plugin.hpp declares WEAK
// (rt_hip_render_tonemapped, rt_hip_tonemap_from_spec), for tests/test_plugin_tonemap.py.
//
// tests/native/plugin_calls.cpp stands for a library that LACKS them: built as it is, the plug-in finds both null.  Linked together with
// this one unit it stands for a library that has them: each fake prints one line per call to stdout in plugin_calls.cpp's style, with
// every argument that is a decision of the plug-in.  The parser is the real one (rt_amd/csrc/tonemap.cpp, included here so that the unit
// stays one), so the parameters printed are what the module would be handed.  Scripted like the other fakes, by call name without the
// rt_hip_ prefix: PLUGIN_CALLS_UNSUPPORTED / PLUGIN_CALLS_FAIL containing render_tonemapped.  Nothing here touches a GPU.
#include "../../rt_amd/csrc/tonemap.cpp"

#include <cinttypes>
#include <string_view>

namespace
{
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

	const char* null_or_set(const void* p) { return p ? "set" : "null"; }
}

extern "C"
{
	rt_hip_status rt_hip_tonemap_from_spec(const char* spec, rt_hip_tonemap_params* out_params)
	{
		const rt_hip::tonemap_check c = rt_hip::tonemap_from_spec(spec, out_params);
		std::printf("rt_hip_tonemap_from_spec spec='%s' out_params=%s -> %d\n", spec ? spec : "(null)", null_or_set(out_params), static_cast<int>(c.status));
		return c.status;
	}

	rt_hip_status rt_hip_render_tonemapped(rt_hip_ctx* ctx, const rt_hip_scene* scene, uint32_t* pixels, uint32_t width, uint32_t height, uint64_t seed, uint32_t flags, const rt_hip_tonemap_params* params, float* rgb_f32,
										   rt_hip_stats* stats, rt_hip_tonemap_info* out_info)
	{
		std::printf("rt_hip_render_tonemapped ctx=%s scene=%s pixels=%s %ux%u seed=%" PRIu64 " flags=0x%x", null_or_set(ctx), null_or_set(scene), null_or_set(pixels), width, height, seed, flags);
		if (params)
			std::printf(" params=curve:%u,low_permille:%u,high_permille:%u,exposure:%g,key:%g,white:%g,min_exposure:%g,max_exposure:%g,adaptation:%g", params->curve, params->low_permille, params->high_permille,
						static_cast<double>(params->exposure), static_cast<double>(params->key), static_cast<double>(params->white), static_cast<double>(params->min_exposure), static_cast<double>(params->max_exposure),
						static_cast<double>(params->adaptation));
		else
			std::printf(" params=null");
		std::printf(" rgb_f32=%s stats=%s out_info=%s", null_or_set(rgb_f32), null_or_set(stats), null_or_set(out_info));
		const rt_hip_status st = listed("PLUGIN_CALLS_UNSUPPORTED", "render_tonemapped") ? RT_HIP_UNSUPPORTED : (listed("PLUGIN_CALLS_FAIL", "render_tonemapped") ? RT_HIP_RUNTIME_ERROR : RT_HIP_OK);
		std::printf(" -> %d\n", static_cast<int>(st));
		return st;
	}
}
