// rt_amd/csrc/lights.cpp — emissive materials' host-only rules (lights.hpp): plain C++17.
#include "lights.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace rt_hip
{
	namespace
	{
		light_check passed()
		{
			light_check c{};
			c.status = RT_HIP_OK;
			return c;
		}

		bool is_blank(char ch) { return ch == ' ' || ch == '\t' || ch == '\n' || ch == '\r'; }
		void trim(const char*& first, const char*& last) // [first, last)
		{
			while (first < last && is_blank(*first))
				first++;
			while (last > first && is_blank(last[-1]))
				last--;
		}

		// "rt_hip_lights_from_spec: item 'KEY=...': why" — the item quoted up to 64 characters
		light_check bad_item(const char* first, const char* last, const char* why)
		{
			light_check c{};
			c.status = RT_HIP_INVALID_ARGUMENT;
			const int shown = static_cast<int>(last - first > 64 ? 64 : last - first);
			std::snprintf(c.message, sizeof c.message, "rt_hip_lights_from_spec: item '%.*s%s': %s", shown, first, last - first > 64 ? "..." : "", why);
			return c;
		}

		// one number, the whole of [first, last): strtof's syntax ("nan" and "inf" parse, and are then refused as values)
		bool parse_number(const char* first, const char* last, float& out)
		{
			trim(first, last);
			const size_t n = static_cast<size_t>(last - first);
			if (!n || n >= 64u)
				return false;
			char text[64];
			std::memcpy(text, first, n);
			text[n] = 0;
			char* end = nullptr;
			out = std::strtof(text, &end);
			return end == text + n;
		}
	}

	light_check check_emission_values(const float* emission_rgb, uint32_t n_materials)
	{
		for (uint32_t m = 0; m < n_materials; m++)
			for (uint32_t k = 0; k < 3u; k++)
			{
				const float v = emission_rgb[m * 3u + k];
				if (!std::isfinite(v) || !(v >= 0.0f)) // (-0.0f >= 0.0f holds: it passes and counts as zero)
				{
					light_check c{};
					c.status = RT_HIP_INVALID_ARGUMENT;
					std::snprintf(c.message, sizeof c.message, "rt_hip_set_emission: material %u, component %c = %g is not a finite number >= 0", m, "rgb"[k], static_cast<double>(v));
					return c;
				}
			}
		return passed();
	}

	uint32_t count_lights(const float* emission_rgb, uint32_t n_materials)
	{
		uint32_t lights = 0;
		for (uint32_t m = 0; m < n_materials; m++)
			lights += is_light(emission_rgb + m * 3u) ? 1u : 0u;
		return lights;
	}

	light_check check_emission_table(const char* entry_point, bool have_table, uint32_t table_rows, uint32_t scene_materials)
	{
		light_check c = passed();
		if (!have_table)
		{
			c.status = RT_HIP_INVALID_ARGUMENT;
			std::snprintf(c.message, sizeof c.message, "%s: RT_HIP_FLAG_EMISSION without an emission table (rt_hip_set_emission)", entry_point);
		}
		else if (table_rows != scene_materials)
		{
			c.status = RT_HIP_INVALID_ARGUMENT;
			std::snprintf(c.message, sizeof c.message, "%s: RT_HIP_FLAG_EMISSION: the emission table has %u rows, the resident scene %u materials", entry_point, table_rows, scene_materials);
		}
		return c;
	}

	light_check lights_from_spec(const char* spec, const char* const* material_names, uint32_t n_materials, float* out_emission_rgb)
	{
		light_check c{};
		c.status = RT_HIP_INVALID_ARGUMENT;
		if (!spec || (n_materials && !out_emission_rgb))
		{
			std::snprintf(c.message, sizeof c.message, "rt_hip_lights_from_spec: NULL argument");
			return c;
		}
		std::vector<float> table(static_cast<size_t>(n_materials) * 3u, 0.0f);
		const char* const spec_end = spec + std::strlen(spec);
		{
			const char *first = spec, *last = spec_end;
			trim(first, last);
			if (first == last) // an empty spec: no light
			{
				if (!table.empty())
					std::memcpy(out_emission_rgb, table.data(), table.size() * sizeof(float));
				return passed();
			}
		}
		for (const char* at = spec;;)
		{
			const char* stop = at;
			while (stop < spec_end && *stop != ';')
				stop++;
			const char *first = at, *last = stop;
			trim(first, last);
			if (first == last)
				return bad_item(first, last, stop == spec_end ? "an empty item (a trailing ';')" : "an empty item");
			const char* equals = first;
			while (equals < last && *equals != '=')
				equals++;
			if (equals == last)
				return bad_item(first, last, "no '=' (KEY=R,G,B or KEY=V)");
			const char *key_first = first, *key_last = equals;
			trim(key_first, key_last);
			if (key_first == key_last)
				return bad_item(first, last, "no key in front of '='");
			// the values: one number (grey) or three
			float rgb[3];
			uint32_t numbers = 0;
			for (const char* v = equals + 1;;)
			{
				const char* comma = v;
				while (comma < last && *comma != ',')
					comma++;
				float value;
				if (!parse_number(v, comma, value))
					return bad_item(first, last, "not a number where one is expected");
				if (numbers == 3u)
					return bad_item(first, last, "more than three numbers (R,G,B or one grey value)");
				rgb[numbers++] = value;
				if (comma == last)
					break;
				v = comma + 1;
			}
			if (numbers == 2u)
				return bad_item(first, last, "two numbers (R,G,B or one grey value)");
			if (numbers == 1u)
				rgb[1] = rgb[2] = rgb[0];
			for (const float value : rgb)
				if (!std::isfinite(value) || !(value >= 0.0f))
					return bad_item(first, last, "a value that is not a finite number >= 0");
			// the key: all digits = a material index; anything else = a name, every material that has it
			bool digits = true;
			for (const char* k = key_first; k < key_last; k++)
				digits = digits && *k >= '0' && *k <= '9';
			if (digits)
			{
				uint64_t index = 0;
				for (const char* k = key_first; k < key_last && index <= 0xFFFFFFFFull; k++)
					index = index * 10u + static_cast<uint64_t>(*k - '0');
				if (index >= n_materials)
					return bad_item(first, last, "material index out of range");
				std::memcpy(&table[static_cast<size_t>(index) * 3u], rgb, sizeof rgb);
			}
			else
			{
				const size_t key_bytes = static_cast<size_t>(key_last - key_first);
				bool found = false;
				for (uint32_t m = 0; material_names && m < n_materials; m++)
					if (material_names[m] && std::strlen(material_names[m]) == key_bytes && std::memcmp(material_names[m], key_first, key_bytes) == 0)
					{
						std::memcpy(&table[static_cast<size_t>(m) * 3u], rgb, sizeof rgb);
						found = true;
					}
				if (!found)
					return bad_item(first, last, "no material of that name");
			}
			if (stop == spec_end)
				break;
			at = stop + 1;
		}
		if (!table.empty())
			std::memcpy(out_emission_rgb, table.data(), table.size() * sizeof(float));
		return passed();
	}
}

extern "C" rt_hip_status rt_hip_lights_from_spec(const char* spec, const char* const* material_names, uint32_t n_materials, float* out_emission_rgb)
{
	try // (the table under construction allocates: nothing may propagate through the C boundary)
	{
		const rt_hip::light_check c = rt_hip::lights_from_spec(spec, material_names, n_materials, out_emission_rgb);
		return c.status ? rt_hip::fail(c.status, "%s", c.message) : RT_HIP_OK;
	}
	catch (...)
	{
		return rt_hip::fail(RT_HIP_RUNTIME_ERROR, "rt_hip_lights_from_spec: out of memory");
	}
}
