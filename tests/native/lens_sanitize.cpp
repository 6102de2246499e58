// tests/native/lens_sanitize.cpp — `make sanitize-lens`: rt_hip_lens_from_spec, the lens' checks and the lens words of a frame
// (rt_amd/csrc/lens.cpp, with rt_amd/csrc/frame_setup.cpp as it is) behind a main() of their own, built with -fsanitize=address,undefined
// and run on the CPU as a plain executable.  The texts of tests/test_lens_host.py, every prefix of a long well-formed spec (truncated
// specs), oversized keys, numbers and item counts, every refused value, and the words of an axis-aligned, a tilted, a 1-pixel frame and
// of matrices without an eye, of zeros and of NaN.  Exits non-zero on the first wrong answer; the sanitizers abort on their own.
#include "../../rt_amd/csrc/lens.hpp"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <string>

namespace
{
	std::string last_message;
	int failures = 0;
}

namespace rt_hip
{
	// what the library's fail() does for its callers: keep the message, hand the status back
	rt_hip_status fail(rt_hip_status status, const char* format, ...)
	{
		char text[512];
		va_list args;
		va_start(args, format);
		std::vsnprintf(text, sizeof text, format, args);
		va_end(args);
		last_message = text;
		return status;
	}
}

namespace
{
	void expect(bool ok, const char* what, const std::string& detail = {})
	{
		if (!ok)
		{
			std::fprintf(stderr, "FAILED: %s %s\n", what, detail.c_str());
			failures++;
		}
	}

	// the spec in a heap block of exactly its size, the lens in one of exactly its own: a stray read or write is the sanitizer's to find
	rt_hip_status parse(const std::string& spec, rt_hip_lens& out)
	{
		std::unique_ptr<char[]> text(new char[spec.size() + 1]);
		std::memcpy(text.get(), spec.c_str(), spec.size() + 1);
		std::unique_ptr<rt_hip_lens> lens(new rt_hip_lens{ -1.0f, -1.0f });
		const rt_hip_status st = rt_hip_lens_from_spec(text.get(), lens.get());
		out = *lens;
		return st;
	}

	void good(const std::string& spec, float aperture, float focus)
	{
		rt_hip_lens lens{};
		const rt_hip_status st = parse(spec, lens);
		expect(st == RT_HIP_OK && lens.aperture_radius == aperture && lens.focus_distance == focus, "accepted", spec);
	}

	void bad(const std::string& spec, const char* why)
	{
		rt_hip_lens lens{};
		last_message.clear();
		const rt_hip_status st = parse(spec, lens);
		expect(st == RT_HIP_INVALID_ARGUMENT && lens.aperture_radius == -1.0f && lens.focus_distance == -1.0f, "refused, lens untouched", spec);
		expect(last_message.rfind("rt_hip_lens_from_spec: ", 0) == 0 && last_message.find(why) != std::string::npos && last_message.size() < 256, "message", spec + " -> " + last_message);
	}

	rt_hip::frame_params frame_of(const float matrix[16], uint32_t width, uint32_t height)
	{
		rt_hip::frame_request wanted{};
		wanted.width = width, wanted.height = height, wanted.partition = { 0, 1, RT_HIP_DEFAULT_STRIPE_ROWS };
		wanted.samples_per_pixel = 4, wanted.max_bounces = 4;
		std::memcpy(wanted.inverse_view_projection, matrix, sizeof wanted.inverse_view_projection);
		return rt_hip::make_frame_params(wanted);
	}
}

int main()
{
	using namespace rt_hip;
	good("aperture=0.05,focus=4.2", 0.05f, 4.2f);
	good("focus=4.2,aperture=0.05", 0.05f, 4.2f);
	good("  aperture = 0.05 ,\tfocus= 4.2 ", 0.05f, 4.2f);
	good("aperture=0,focus=1e-3", 0.0f, 1e-3f);
	good("aperture=1e3,focus=0x1p2", 1000.0f, 4.0f);
	bad("", "an empty item");
	bad("aperture=0.05", "'focus' is missing");
	bad("focus=2", "'aperture' is missing");
	bad("aperture=0.05,", "an empty item");
	bad("aperture=0.05,,focus=1", "an empty item");
	bad("aperture=0.05,focus", "no '='");
	bad("aperture=0.05,focus=", "not a number");
	bad("aperture=0.05,focus=4.2x", "not a number");
	bad("aperture=0.05,focus=4.2,aperture=0.1", "a key given twice");
	bad("aperture=0.05,focus=4.2,blades=6", "an unknown key");
	bad("=0.05,focus=4.2", "an unknown key");
	bad("aperture=-0.05,focus=4.2", "aperture_radius");
	bad("aperture=nan,focus=4.2", "aperture_radius");
	bad("aperture=0.05,focus=0", "focus_distance");
	bad("aperture=0.05,focus=inf", "focus_distance");
	bad("aperture=" + std::string(80, '9') + ",focus=1", "not a number");
	bad("focus=1,aperture=0.05," + std::string(5000, 'x'), "no '='");
	bad(std::string(5000, ','), "an empty item");
	bad(std::string(300, 'k') + "=1,focus=1", "an unknown key");
	{
		// every prefix of a well-formed spec: accepted or refused, never a stray read
		const std::string whole = " aperture = 0.125 , focus = 17.5e-1 ";
		for (size_t n = 0; n <= whole.size(); n++)
		{
			rt_hip_lens lens{};
			const rt_hip_status st = parse(whole.substr(0, n), lens);
			expect(st == RT_HIP_OK || st == RT_HIP_INVALID_ARGUMENT, "a truncated spec", whole.substr(0, n));
		}
		rt_hip_lens lens{};
		expect(rt_hip_lens_from_spec(nullptr, &lens) == RT_HIP_INVALID_ARGUMENT && rt_hip_lens_from_spec("aperture=1,focus=1", nullptr) == RT_HIP_INVALID_ARGUMENT, "NULL arguments");
	}
	{
		const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
		const struct
		{
			float aperture, focus;
			const char* field; // NULL: accepted
		} lenses[] = { { 0.0f, 1.0f, nullptr },		  { -0.0f, 1e-30f, nullptr },		{ 1000.0f, 1e-3f, nullptr },		{ -1.0f, 1.0f, "aperture_radius" }, { nan, 1.0f, "aperture_radius" },
					   { inf, 1.0f, "aperture_radius" }, { 0.1f, 0.0f, "focus_distance" }, { 0.1f, -2.0f, "focus_distance" }, { 0.1f, nan, "focus_distance" },		{ 0.1f, inf, "focus_distance" } };
		for (const auto& l : lenses)
		{
			const lens_check c = check_lens("rt_hip_set_lens", rt_hip_lens{ l.aperture, l.focus });
			expect(l.field ? (c.status == RT_HIP_INVALID_ARGUMENT && std::strstr(c.message, l.field) != nullptr) : c.status == RT_HIP_OK, "check_lens", c.message);
		}
	}
	{
		// rt's axis-aligned camera at (0, 1, 3) looking down -z (near 0.1, far 1000, 64 x 36), the same tilted, and matrices that are no camera's
		const float axis[16] = { 0.73638f, 0, 0, 0, 0, 0.41421f, 0, 1.0f, 0, 0, 0, 2.0f, 0, 0, -4.9995f, 5.0005f };
		const float tilted[16] = { 0.72f, 0.05f, 0.14f, 0.3f, -0.02f, 0.40f, -0.10f, 1.5f, -0.15f, 0.08f, 0.6f, 4.0f, 0.001f, -0.002f, -4.9995f, 5.0005f };
		const float flat[16] = { 2.4f, 0, 0, 0, 0, 1.35f, 0, 1, 0, 0, -12, 3, 0, 0, 0, 1 };
		const float zeros[16] = {};
		float nans[16];
		for (float& v : nans)
			v = std::numeric_limits<float>::quiet_NaN();
		const rt_hip_lens lens = { 0.125f, 4.2f };
		const struct
		{
			const float* matrix;
			uint32_t width, height;
			bool has_eye;
		} frames[] = { { axis, 64, 36, true }, { tilted, 64, 36, true }, { tilted, 1, 1, true }, { axis, 1, 131070, true }, { flat, 64, 36, false }, { zeros, 64, 36, false }, { nans, 64, 36, false } };
		for (const auto& f : frames)
		{
			const frame_params p = frame_of(f.matrix, f.width, f.height);
			const lens_check with = check_lens_frame("rt_hip_render_device", true, p), without = check_lens_frame("rt_hip_render_device", false, p);
			expect(without.status == RT_HIP_INVALID_ARGUMENT && std::strstr(without.message, "rt_hip_set_lens") != nullptr, "a frame without a lens");
			expect(f.has_eye ? with.status == RT_HIP_OK : (with.status == RT_HIP_UNSUPPORTED && std::strstr(with.message, "RT_HIP_FLAG_THIN_LENS") != nullptr), "a frame's camera", with.message);
			const lens_words w = make_lens_words(p, f.matrix, lens); // (made whatever the check said: no stray access for any matrix)
			frame_params carrier = p;
			put_lens_words(carrier, w);
			expect(carrier.mx[3] == lens.focus_distance && carrier.k_near[3] == 0.0f && carrier.k_far[0] == 0.0f, "the words' places");
			if (f.has_eye)
			{
				const double u = std::sqrt(double(w.u[0]) * w.u[0] + double(w.u[1]) * w.u[1] + double(w.u[2]) * w.u[2]);
				const double n = std::sqrt(double(w.fwd[0]) * w.fwd[0] + double(w.fwd[1]) * w.fwd[1] + double(w.fwd[2]) * w.fwd[2]);
				const double across = double(w.u[0]) * w.fwd[0] + double(w.u[1]) * w.fwd[1] + double(w.u[2]) * w.fwd[2];
				expect(std::fabs(u - lens.aperture_radius) < 1e-6 && std::fabs(n - 1.0) < 1e-6 && std::fabs(across) < 1e-6, "U has the aperture's length, fwd is a unit vector across it");
			}
		}
	}
	if (failures)
		return 1;
	std::puts("lens_sanitize: all answers as expected");
	return 0;
}
