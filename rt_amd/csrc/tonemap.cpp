// rt_amd/csrc/tonemap.cpp — tone mapping's parameters and the CURVE[:EXPOSURE] parser (tonemap.hpp): host-only, plain C++17.
#include "tonemap.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace rt_hip
{
	// Conventional values, not tuned ones: the middle grey of photography, a rank window that ignores the darkest twentieth and the
	// brightest fiftieth of the metered pixels (a lamp in view must not set the exposure), ten stops either way.
	rt_hip_tonemap_params default_tonemap_params()
	{
		rt_hip_tonemap_params p{};
		p.curve = RT_HIP_TONEMAP_ACES;
		p.low_permille = 50;
		p.high_permille = 20;
		p.exposure = 0.0f;
		p.key = 0.18f;
		p.white = 4.0f;
		p.min_exposure = 0.0009765625f; // 2^-10
		p.max_exposure = 1024.0f;
		p.adaptation = 1.0f;
		return p;
	}

	tonemap_check check_tonemap_params(const rt_hip_tonemap_params& p)
	{
		tonemap_check c{};
		c.status = RT_HIP_OK;
		const auto refuse = [&c](const char* field, const char* why, double value)
		{
			c.status = RT_HIP_INVALID_ARGUMENT;
			std::snprintf(c.message, sizeof c.message, "rt_hip_tonemap_params: %s = %g %s", field, value, why);
		};
		const auto positive = [](float v) { return std::isfinite(v) && v > 0.0f; };
		if (p.curve > RT_HIP_TONEMAP_ACES)
			refuse("curve", "is not 0 (none), 1 (reinhard) or 2 (aces)", p.curve);
		else if (p.low_permille >= 1000u)
			refuse("low_permille", "is not below 1000", p.low_permille);
		else if (p.high_permille >= 1000u || p.low_permille + p.high_permille >= 1000u)
			refuse("high_permille", "leaves no pixel: low_permille + high_permille must be below 1000", p.high_permille);
		else if (p.exposure != 0.0f && !positive(p.exposure))
			refuse("exposure", "is neither 0 (auto) nor a positive finite number", p.exposure);
		else if (!positive(p.key))
			refuse("key", "is not a positive finite number", p.key);
		else if (!(p.white >= 0x1p-20f) || !(p.white <= 0x1p20f)) // (white^2 stays a normal float, and no quotient by it overflows)
			refuse("white", "is not in [2^-20, 2^20]", p.white);
		else if (!positive(p.min_exposure))
			refuse("min_exposure", "is not a positive finite number", p.min_exposure);
		else if (!positive(p.max_exposure) || p.max_exposure < p.min_exposure)
			refuse("max_exposure", "is not a positive finite number that is at least min_exposure", p.max_exposure);
		else if (!(p.adaptation > 0.0f) || !(p.adaptation <= 1.0f))
			refuse("adaptation", "is not in (0, 1]", p.adaptation);
		return c;
	}

	tonemap_check tonemap_from_spec(const char* spec, rt_hip_tonemap_params* out)
	{
		tonemap_check c{};
		c.status = RT_HIP_OK;
		if (!spec || !out)
		{
			c.status = RT_HIP_INVALID_ARGUMENT;
			std::snprintf(c.message, sizeof c.message, "rt_hip_tonemap_from_spec: NULL argument");
			return c;
		}
		const auto refuse = [&c, spec](const char* why)
		{
			c.status = RT_HIP_INVALID_ARGUMENT; // (the text quoted up to 64 characters)
			std::snprintf(c.message, sizeof c.message, "rt_hip_tonemap_from_spec: '%.64s%s': %s", spec, std::strlen(spec) > 64 ? "..." : "", why);
		};
		rt_hip_tonemap_params p = default_tonemap_params();
		const char* const colon = std::strchr(spec, ':');
		const size_t name = colon ? static_cast<size_t>(colon - spec) : std::strlen(spec);
		const auto is = [&](const char* word) { return std::strlen(word) == name && std::memcmp(spec, word, name) == 0; };
		if (is("none"))
			p.curve = RT_HIP_TONEMAP_NONE;
		else if (is("reinhard"))
			p.curve = RT_HIP_TONEMAP_REINHARD;
		else if (is("aces"))
			p.curve = RT_HIP_TONEMAP_ACES;
		else
		{
			refuse("the curve is none, reinhard or aces");
			return c;
		}
		if (colon && std::strcmp(colon + 1, "auto") != 0)
		{
			const char* const text = colon + 1;
			char* end = nullptr;
			const float value = std::strtof(text, &end);
			// (strtof takes blanks, signs, hexadecimal, "inf" and "nan": a number here starts with a digit or a point, is decimal and finite)
			const bool plain = ((*text >= '0' && *text <= '9') || *text == '.') && std::strspn(text, "0123456789.eE+-") == std::strlen(text);
			if (!plain || end == text || *end || !std::isfinite(value) || !(value > 0.0f))
			{
				refuse("the exposure is auto or a positive number");
				return c;
			}
			p.exposure = value;
		}
		*out = p;
		return c;
	}
}
