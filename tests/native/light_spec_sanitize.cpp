// tests/native/light_spec_sanitize.cpp — `make sanitize-lights`: rt_hip_lights_from_spec and the emission table's checks
// (rt_amd/csrc/lights.cpp) behind a main() of their own, built with -fsanitize=address,undefined and run on the CPU as a plain
// executable.  The cases of tests/test_light_spec.py, every prefix of a long well-formed spec (truncated specs), oversized keys, numbers
// and item counts, and tables with every kind of bad value.  Exits non-zero on the first wrong answer; the sanitizers abort on their own.
#include "../../rt_amd/csrc/lights.hpp"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

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
	const char* const names[5] = { "ground", "lamp", "clay", "lamp", "glass" };

	void expect(bool ok, const char* what, const std::string& detail = {})
	{
		if (!ok)
		{
			std::fprintf(stderr, "FAILED: %s %s\n", what, detail.c_str());
			failures++;
		}
	}

	// exactly 15 floats behind a heap block of exactly that size: an out-of-bounds write is the sanitizer's to find
	rt_hip_status parse(const std::string& spec, std::vector<float>& out, bool with_names = true)
	{
		out.assign(15, 7.0f);
		out.shrink_to_fit();
		return rt_hip_lights_from_spec(spec.c_str(), with_names ? names : nullptr, 5, out.data());
	}

	void good(const std::string& spec, std::initializer_list<float> want)
	{
		std::vector<float> out;
		const rt_hip_status st = parse(spec, out);
		expect(st == RT_HIP_OK, "a well-formed spec is refused:", spec + " -> " + last_message);
		expect(st != RT_HIP_OK || std::equal(want.begin(), want.end(), out.begin()), "a well-formed spec gives another table:", spec);
	}

	void bad(const std::string& spec, const char* why, bool with_names = true)
	{
		std::vector<float> out;
		const rt_hip_status st = parse(spec, out, with_names);
		expect(st == RT_HIP_INVALID_ARGUMENT, "a malformed spec is not refused:", spec);
		expect(last_message.find(why) != std::string::npos, "the refusal does not say why:", spec + " -> " + last_message);
		for (const float v : out)
			expect(v == 7.0f, "a refused spec touched the output:", spec);
	}
}

int main()
{
	using namespace rt_hip;
	good("", { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 });
	good(" \t\n", { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 });
	good("1=4,3.5,2", { 0, 0, 0, 4, 3.5f, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0 });
	good("lamp=3", { 0, 0, 0, 3, 3, 3, 0, 0, 0, 3, 3, 3, 0, 0, 0 });
	good("  lamp = 4 , 3.5 ,2 ;\t0=1 ", { 1, 1, 1, 4, 3.5f, 2, 0, 0, 0, 4, 3.5f, 2, 0, 0, 0 });
	good("lamp=1,1,1;3=2,2,2;004=0x1p-2", { 0, 0, 0, 1, 1, 1, 0, 0, 0, 2, 2, 2, 0.25f, 0.25f, 0.25f });
	bad("lantern=1,1,1", "no material of that name");
	bad("lamp=1", "no material of that name", false);
	bad("5=1,1,1", "out of range");
	bad("99999999999999999999=1", "out of range");
	bad("lamp=1,2", "two numbers");
	bad("lamp=1,2,3,4", "more than three");
	bad("lamp=1,-2,3", "finite number >= 0");
	bad("lamp=nan", "finite number >= 0");
	bad("0=1,inf,1", "finite number >= 0");
	bad("0=1e39", "finite number >= 0");
	bad("lamp 1,1,1", "no '='");
	bad("lamp=1;", "trailing ';'");
	bad("lamp=1;;0=1", "empty item");
	bad(";", "empty item");
	bad("=1,1,1", "no key");
	bad("lamp=", "not a number");
	bad("lamp=1,,1", "not a number");
	bad("lamp=1x", "not a number");
	bad("0=1;lamp=1,2", "two numbers");

	// truncated: every prefix of a well-formed spec is accepted or refused, never anything else
	const std::string whole = " lamp = 4 , 3.5 ,2 ; 0=1e-3;glass=0x1.8p1,0,0 ;2=0.5";
	for (size_t cut = 0; cut <= whole.size(); cut++)
	{
		std::vector<float> out;
		const rt_hip_status st = parse(whole.substr(0, cut), out);
		expect(st == RT_HIP_OK || st == RT_HIP_INVALID_ARGUMENT, "a truncated spec gives another status");
	}
	// oversized: a key, a number and a name far beyond any buffer of the parser's; thousands of items; a long run of separators
	bad(std::string(100000, 'x') + "=1", "no material of that name");
	bad("0=" + std::string(100000, '1'), "not a number");
	bad("0=1," + std::string(5000, ' ') + "x", "not a number");
	bad(std::string(10000, ';'), "empty item");
	{
		std::string many;
		for (int i = 0; i < 20000; i++)
			many += (i ? ";" : "") + std::to_string(i % 5) + "=" + std::to_string(i);
		std::vector<float> out;
		expect(parse(many, out) == RT_HIP_OK && out[12] == 19999.0f, "twenty thousand items");
	}
	{
		// no materials at all: nothing is written, nothing is read
		expect(rt_hip_lights_from_spec("", nullptr, 0, nullptr) == RT_HIP_OK, "an empty spec for no materials");
		expect(rt_hip_lights_from_spec("0=1", nullptr, 0, nullptr) == RT_HIP_INVALID_ARGUMENT, "an index for no materials");
		expect(rt_hip_lights_from_spec(nullptr, names, 5, nullptr) == RT_HIP_INVALID_ARGUMENT, "a NULL spec");
		const char* const holes[3] = { "a", nullptr, "b" }; // a NULL name matches nothing
		float out[9];
		expect(rt_hip_lights_from_spec("b=1", holes, 3, out) == RT_HIP_OK && out[6] == 1.0f && out[3] == 0.0f, "a NULL among the names");
	}

	// the table's own checks
	{
		const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
		std::vector<float> t = { 0, 0, 0, 4, 3.5f, 2, -0.0f, 0, 0 };
		t.shrink_to_fit();
		expect(check_emission_values(t.data(), 3).status == RT_HIP_OK, "a good table is refused");
		expect(count_lights(t.data(), 3) == 1u, "one light (-0 is no light)");
		expect(check_emission_values(nullptr, 0).status == RT_HIP_OK && count_lights(nullptr, 0) == 0u, "the empty table");
		const struct
		{
			float value;
			uint32_t at;
			const char* names_it;
		} wrong[] = { { -1.0f, 5, "material 1, component b" }, { nan, 0, "material 0, component r" }, { inf, 7, "material 2, component g" }, { -inf, 8, "material 2, component b" } };
		for (const auto& w : wrong)
		{
			std::vector<float> u = t;
			u[w.at] = w.value;
			const light_check c = check_emission_values(u.data(), 3);
			expect(c.status == RT_HIP_INVALID_ARGUMENT && std::strstr(c.message, w.names_it), "a bad component is not named:", c.message);
		}
		expect(check_emission_table("here", false, 0, 5).status == RT_HIP_INVALID_ARGUMENT, "no table");
		const light_check rows = check_emission_table("here", true, 7, 5);
		expect(rows.status == RT_HIP_INVALID_ARGUMENT && std::strstr(rows.message, "7 rows") && std::strstr(rows.message, "5 materials"), "another scene's table");
		expect(check_emission_table("here", true, 5, 5).status == RT_HIP_OK, "the scene's table");
	}
	if (failures)
		return 1;
	std::puts("light_spec_sanitize: every case as expected");
	return 0;
}
