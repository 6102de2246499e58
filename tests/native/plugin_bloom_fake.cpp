// tests/native/plugin_bloom_fake.cpp — recording fakes of the two entry points shim/rt_hip_plugin.hpp declares WEAK for bloom
// (rt_hip_render_bloomed, rt_hip_bloom_from_spec), for tests/test_plugin_bloom.py.
//
// It brings tests/native/plugin_tonemap_fake.cpp along (included, so that the unit stays one): a library that has bloom has tone mapping.
// tests/native/plugin_calls.cpp alone, or with plugin_tonemap_fake.cpp, stands for a library that LACKS the call.  Each fake prints one
// line per call to stdout in plugin_calls.cpp's style, with every argument that is a decision of the plug-in.  The parser is the real one
// (rt_amd/csrc/bloom.cpp, included here).  Scripted like the other fakes: PLUGIN_CALLS_UNSUPPORTED / PLUGIN_CALLS_FAIL containing
// render_bloomed.  Nothing here touches a GPU.
#include "plugin_tonemap_fake.cpp"
#include "../../rt_amd/csrc/bloom.cpp"

extern "C"
{
	rt_hip_status rt_hip_bloom_from_spec(const char* spec, rt_hip_bloom_params* out_params)
	{
		const rt_hip::bloom_check c = rt_hip::bloom_from_spec(spec, out_params);
		std::printf("rt_hip_bloom_from_spec spec='%s' out_params=%s -> %d\n", spec ? spec : "(null)", null_or_set(out_params), static_cast<int>(c.status));
		if (c.status) // (what the module would leave in rt_hip_last_error: plugin_calls.cpp's own is out of this unit's reach)
			std::printf("message %s\n", c.message);
		return c.status;
	}

	rt_hip_status rt_hip_render_bloomed(rt_hip_ctx* ctx, const rt_hip_scene* scene, uint32_t* pixels, uint32_t width, uint32_t height, uint64_t seed, uint32_t flags, const rt_hip_bloom_params* bloom_params,
										const rt_hip_tonemap_params* tonemap_params, float* rgb_f32, rt_hip_stats* stats, rt_hip_tonemap_info* out_info)
	{
		std::printf("rt_hip_render_bloomed ctx=%s scene=%s pixels=%s %ux%u seed=%" PRIu64 " flags=0x%x", null_or_set(ctx), null_or_set(scene), null_or_set(pixels), width, height, seed, flags);
		if (bloom_params)
			std::printf(" bloom=threshold:%g,knee:%g,intensity:%g,scatter:%g,levels:%u", static_cast<double>(bloom_params->threshold), static_cast<double>(bloom_params->knee), static_cast<double>(bloom_params->intensity),
						static_cast<double>(bloom_params->scatter), bloom_params->levels);
		else
			std::printf(" bloom=null");
		if (tonemap_params)
			std::printf(" tonemap=curve:%u,exposure:%g,adaptation:%g", tonemap_params->curve, static_cast<double>(tonemap_params->exposure), static_cast<double>(tonemap_params->adaptation));
		else
			std::printf(" tonemap=null");
		std::printf(" rgb_f32=%s stats=%s out_info=%s", null_or_set(rgb_f32), null_or_set(stats), null_or_set(out_info));
		const rt_hip_status st = listed("PLUGIN_CALLS_UNSUPPORTED", "render_bloomed") ? RT_HIP_UNSUPPORTED : (listed("PLUGIN_CALLS_FAIL", "render_bloomed") ? RT_HIP_RUNTIME_ERROR : RT_HIP_OK);
		std::printf(" -> %d\n", static_cast<int>(st));
		return st;
	}
}
