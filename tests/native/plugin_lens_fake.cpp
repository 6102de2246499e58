// tests/native/plugin_lens_fake.cpp — recording fakes of the two entry points shim/rt_hip_plugin.hpp declares WEAK for the thin lens
// (rt_hip_set_lens, rt_hip_lens_from_spec), for tests/test_plugin_lens.py.
//
// It brings tests/native/plugin_bloom_fake.cpp along (included, so that the unit stays one): a library that has the lens has bloom and tone
// mapping.  tests/native/plugin_calls.cpp alone, or with one of the older fakes, stands for a library that LACKS the calls.  Each fake
// prints one line per call to stdout in plugin_calls.cpp's style, with every argument that is a decision of the plug-in.  The parser and
// the check are the real ones (rt_amd/csrc/lens.cpp, included here with its own C entry point under another name).  Scripted like the
// other fakes: PLUGIN_CALLS_FAIL containing set_lens.  Nothing here touches a GPU.
#include "plugin_bloom_fake.cpp"

namespace rt_hip
{
	// (lens.cpp's own C entry point reports through the library's fail(); nothing here calls it)
	rt_hip_status fail(rt_hip_status status, const char*, ...) { return status; }
}
#define rt_hip_lens_from_spec rt_hip_lens_from_spec_of_the_library
#include "../../rt_amd/csrc/lens.cpp"
#undef rt_hip_lens_from_spec

extern "C"
{
	rt_hip_status rt_hip_lens_from_spec(const char* spec, rt_hip_lens* out_lens)
	{
		const rt_hip::lens_check c = rt_hip::lens_from_spec(spec, out_lens);
		std::printf("rt_hip_lens_from_spec spec='%s' out_lens=%s -> %d\n", spec ? spec : "(null)", null_or_set(out_lens), static_cast<int>(c.status));
		if (c.status) // (what the module would leave in rt_hip_last_error: plugin_calls.cpp's own is out of this unit's reach)
			std::printf("message %s\n", c.message);
		return c.status;
	}

	rt_hip_status rt_hip_set_lens(rt_hip_ctx* ctx, const rt_hip_lens* lens)
	{
		std::printf("rt_hip_set_lens ctx=%s", null_or_set(ctx));
		if (lens)
			std::printf(" lens=aperture:%g,focus:%g", static_cast<double>(lens->aperture_radius), static_cast<double>(lens->focus_distance));
		else
			std::printf(" lens=null");
		const rt_hip_status st = listed("PLUGIN_CALLS_FAIL", "set_lens") ? RT_HIP_RUNTIME_ERROR : RT_HIP_OK;
		std::printf(" -> %d\n", static_cast<int>(st));
		return st;
	}
}
