// rt_amd/csrc/bloom.cpp — bloom's parameters, the level plan and the key=value parser (bloom.hpp): host-only, plain C++17.
#include "bloom.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace rt_hip
{
	// Conventional values, not tuned ones: what lies above display white glows, through a knee half as wide, a tenth of it is added.
	rt_hip_bloom_params default_bloom_params()
	{
		rt_hip_bloom_params p{};
		p.threshold = 1.0f;
		p.knee = 0.5f;
		p.intensity = 0.1f;
		p.scatter = 0.7f;
		p.levels = 6;
		return p;
	}

	// (every comparison is written so that a NaN fails it)
	bloom_check check_bloom_params(const rt_hip_bloom_params& p)
	{
		bloom_check c{};
		c.status = RT_HIP_OK;
		const auto refuse = [&c](const char* field, const char* why, double value)
		{
			c.status = RT_HIP_INVALID_ARGUMENT;
			std::snprintf(c.message, sizeof c.message, "rt_hip_bloom_params: %s = %g %s", field, value, why);
		};
		if (!(p.threshold >= 0.0f) || !(p.threshold <= 0x1p20f))
			refuse("threshold", "is not in [0, 2^20]", p.threshold);
		else if (p.knee != 0.0f && (!(p.knee >= 0x1p-20f) || !(p.knee <= p.threshold))) // (4 knee is a normal divisor; a black pixel stays black)
			refuse("knee", "is neither 0 nor in [2^-20, threshold]", p.knee);
		else if (!(p.intensity >= 0.0f) || !(p.intensity <= 1024.0f))
			refuse("intensity", "is not in [0, 2^10]", p.intensity);
		else if (!(p.scatter >= 0.0f) || !(p.scatter <= 1.0f))
			refuse("scatter", "is not in [0, 1]", p.scatter);
		else if (p.levels < 1u || p.levels > bloom::max_levels)
			refuse("levels", "is not in 1 .. 8", p.levels);
		return c;
	}

	bloom_plan plan_bloom(uint32_t width, uint32_t height, const rt_hip_bloom_params& p)
	{
		bloom_plan plan{};
		uint32_t w = width, h = height;
		size_t offset = 0;
		while (plan.levels < p.levels)
		{
			w = bloom::half_up(w), h = bloom::half_up(h);
			plan.level[plan.levels++] = { w, h, offset };
			offset += static_cast<size_t>(w) * h * 3u;
			if (w == 1u && h == 1u)
				break;
		}
		float norm = 0.0f, term = 1.0f;
		for (uint32_t i = 0; i < plan.levels; i++)
		{
			norm += term;
			term *= p.scatter;
		}
		plan.norm = norm;
		plan.gain = p.intensity / norm;
		plan.scratch_bytes = offset * sizeof(float);
		return plan;
	}

	bloom_check bloom_from_spec(const char* spec, rt_hip_bloom_params* out)
	{
		bloom_check c{};
		c.status = RT_HIP_OK;
		if (!spec || !out)
		{
			c.status = RT_HIP_INVALID_ARGUMENT;
			std::snprintf(c.message, sizeof c.message, "rt_hip_bloom_from_spec: NULL argument");
			return c;
		}
		const auto refuse = [&c, spec](const char* why)
		{
			c.status = RT_HIP_INVALID_ARGUMENT; // (the text quoted up to 64 characters)
			std::snprintf(c.message, sizeof c.message, "rt_hip_bloom_from_spec: '%.64s%s': %.100s", spec, std::strlen(spec) > 64 ? "..." : "", why);
		};
		rt_hip_bloom_params p = default_bloom_params();
		if (std::strcmp(spec, "default") != 0)
		{
			static const char* const keys[] = { "intensity", "threshold", "knee", "scatter", "levels" };
			bool given[5] = {};
			const char* item = spec;
			for (;;)
			{
				const char* const end = std::strchr(item, ',') ? std::strchr(item, ',') : item + std::strlen(item);
				const char* const equals = static_cast<const char*>(std::memchr(item, '=', static_cast<size_t>(end - item)));
				if (!equals)
				{
					refuse("an item is KEY=VALUE, the items are separated by ',' (or the whole text is default)");
					return c;
				}
				size_t key = 0;
				while (key < 5u && !(std::strlen(keys[key]) == static_cast<size_t>(equals - item) && std::memcmp(item, keys[key], static_cast<size_t>(equals - item)) == 0))
					key++;
				if (key == 5u)
				{
					refuse("the keys are intensity, threshold, knee, scatter and levels");
					return c;
				}
				if (given[key])
				{
					refuse("a key is given twice");
					return c;
				}
				given[key] = true;
				// (strtof takes blanks, signs, hexadecimal, "inf" and "nan": a number here starts with a digit or a point, is decimal and finite)
				char text[32] = {};
				const size_t length = static_cast<size_t>(end - (equals + 1));
				if (length == 0u || length >= sizeof text)
				{
					refuse("a value is a plain decimal number");
					return c;
				}
				std::memcpy(text, equals + 1, length);
				char* stop = nullptr;
				const float value = std::strtof(text, &stop);
				const bool plain = ((*text >= '0' && *text <= '9') || *text == '.') && std::strspn(text, "0123456789.eE+-") == length;
				if (!plain || stop == text || *stop || !std::isfinite(value))
				{
					refuse("a value is a plain decimal number");
					return c;
				}
				if (key == 4u)
				{
					if (std::strspn(text, "0123456789") != length || !(value <= 1e6f))
					{
						refuse("levels is a whole number");
						return c;
					}
					p.levels = static_cast<uint32_t>(value);
				}
				else
					(key == 0u ? p.intensity : key == 1u ? p.threshold : key == 2u ? p.knee : p.scatter) = value;
				if (!*end)
					break;
				item = end + 1;
			}
		}
		if (const bloom_check checked = check_bloom_params(p); checked.status)
		{
			refuse(checked.message);
			return c;
		}
		*out = p;
		return c;
	}
}
