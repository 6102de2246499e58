// rt_amd/csrc/lens.cpp — the thin lens' host-only rules (lens.hpp): plain C++17.  Built with -ffp-contract=off: the binary64 constants
// below are defined by their order of operations.
#include "lens.hpp"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace rt_hip
{
	namespace
	{
		lens_check passed()
		{
			lens_check c{};
			c.status = RT_HIP_OK;
			return c;
		}

		__attribute__((format(printf, 2, 3))) lens_check refused(rt_hip_status status, const char* format, ...)
		{
			lens_check c{};
			c.status = status;
			va_list args;
			va_start(args, format);
			std::vsnprintf(c.message, sizeof c.message, format, args);
			va_end(args);
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

		// "rt_hip_lens_from_spec: item 'aperture=...': why" — the item quoted up to 64 characters
		lens_check bad_item(const char* first, const char* last, const char* why)
		{
			const int shown = static_cast<int>(last - first > 64 ? 64 : last - first);
			return refused(RT_HIP_INVALID_ARGUMENT, "rt_hip_lens_from_spec: item '%.*s%s': %s", shown, first, last - first > 64 ? "..." : "", why);
		}
	}

	lens_check check_lens(const char* entry_point, const rt_hip_lens& lens)
	{
		if (!std::isfinite(lens.aperture_radius) || !(lens.aperture_radius >= 0.0f)) // (-0.0f passes and counts as zero)
			return refused(RT_HIP_INVALID_ARGUMENT, "%s: aperture_radius = %g is not a finite number >= 0", entry_point, static_cast<double>(lens.aperture_radius));
		if (!std::isfinite(lens.focus_distance) || !(lens.focus_distance > 0.0f))
			return refused(RT_HIP_INVALID_ARGUMENT, "%s: focus_distance = %g is not a finite number > 0", entry_point, static_cast<double>(lens.focus_distance));
		return passed();
	}

	lens_check check_lens_frame(const char* entry_point, bool have_lens, const frame_params& frame)
	{
		if (!have_lens)
			return refused(RT_HIP_INVALID_ARGUMENT, "%s: RT_HIP_FLAG_THIN_LENS without a lens (rt_hip_set_lens)", entry_point);
		if (!frame.pinhole && !frame.eye_form)
			return refused(RT_HIP_UNSUPPORTED, "%s: RT_HIP_FLAG_THIN_LENS needs a perspective matrix: this frame's has no finite eye", entry_point);
		return passed();
	}

	lens_check lens_from_spec(const char* spec, rt_hip_lens* out_lens)
	{
		if (!spec || !out_lens)
			return refused(RT_HIP_INVALID_ARGUMENT, "rt_hip_lens_from_spec: NULL argument");
		const char* const spec_end = spec + std::strlen(spec);
		float values[2] = { 0.0f, 0.0f }; // aperture, focus
		bool seen[2] = { false, false };
		static const char* const keys[2] = { "aperture", "focus" };
		for (const char* at = spec;;)
		{
			const char* stop = at;
			while (stop < spec_end && *stop != ',')
				stop++;
			const char *first = at, *last = stop;
			trim(first, last);
			if (first == last)
				return bad_item(first, last, "an empty item");
			const char* equals = first;
			while (equals < last && *equals != '=')
				equals++;
			if (equals == last)
				return bad_item(first, last, "no '=' (aperture=A,focus=F)");
			const char *key_first = first, *key_last = equals;
			trim(key_first, key_last);
			const size_t key_bytes = static_cast<size_t>(key_last - key_first);
			int which = -1;
			for (int k = 0; k < 2; k++)
				if (std::strlen(keys[k]) == key_bytes && std::memcmp(keys[k], key_first, key_bytes) == 0)
					which = k;
			if (which < 0)
				return bad_item(first, last, "an unknown key (aperture, focus)");
			if (seen[which])
				return bad_item(first, last, "a key given twice");
			if (!parse_number(equals + 1, last, values[which]))
				return bad_item(first, last, "not a number where one is expected");
			seen[which] = true;
			if (stop == spec_end)
				break;
			at = stop + 1;
		}
		if (!seen[0] || !seen[1])
			return refused(RT_HIP_INVALID_ARGUMENT, "rt_hip_lens_from_spec: '%s' is missing (aperture=A,focus=F)", seen[0] ? keys[1] : keys[0]);
		const rt_hip_lens lens = { values[0], values[1] };
		const lens_check values_ok = check_lens("rt_hip_lens_from_spec", lens);
		if (values_ok.status)
			return values_ok;
		*out_lens = lens;
		return passed();
	}

	lens_words make_lens_words(const frame_params& frame, const float M[16], const rt_hip_lens& lens)
	{
		// near(px, py) = (M (X, Y, 0, 1)).xyz / w with X = (2 / W) px - 1, Y = -(2 / H) py + 1, in binary64
		const double sx = 2.0 / static_cast<double>(frame.width), sy = -(2.0 / static_cast<double>(frame.height));
		const auto near_point = [&](double px, double py, double out[3])
		{
			const double X = sx * px - 1.0, Y = sy * py + 1.0;
			double row[4];
			for (int r = 0; r < 4; r++)
				row[r] = static_cast<double>(M[r * 4 + 0]) * X + static_cast<double>(M[r * 4 + 1]) * Y + static_cast<double>(M[r * 4 + 3]);
			for (int c = 0; c < 3; c++)
				out[c] = row[c] / row[3];
		};
		const auto normalise = [](double v[3])
		{
			const double length = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
			for (int c = 0; c < 3; c++)
				v[c] = v[c] / length;
		};
		const double cx = 0.5 * static_cast<double>(frame.width), cy = 0.5 * static_cast<double>(frame.height);
		double centre[3], beside[3], below[3];
		near_point(cx, cy, centre);
		near_point(cx + 1.0, cy, beside);
		near_point(cx, cy + 1.0, below);
		double right[3], up[3], fwd[3];
		for (int c = 0; c < 3; c++)
			right[c] = beside[c] - centre[c], up[c] = -(below[c] - centre[c]);
		normalise(right);
		normalise(up);
		fwd[0] = right[1] * up[2] - right[2] * up[1];
		fwd[1] = right[2] * up[0] - right[0] * up[2];
		fwd[2] = right[0] * up[1] - right[1] * up[0];
		normalise(fwd);
		const float* const eye = frame.pinhole ? frame.ray_eye : frame.eye_e;
		double ahead = 0.0;
		for (int c = 0; c < 3; c++)
			ahead += fwd[c] * (centre[c] - static_cast<double>(eye[c]));
		if (!(ahead > 0.0))
			for (int c = 0; c < 3; c++)
				fwd[c] = -fwd[c];
		lens_words w{};
		const double aperture = lens.aperture_radius;
		for (int c = 0; c < 3; c++)
		{
			w.u[c] = static_cast<float>(aperture * right[c]);
			w.v[c] = static_cast<float>(aperture * up[c]);
			w.fwd[c] = static_cast<float>(fwd[c]);
		}
		w.focus = lens.focus_distance;
		return w;
	}

	void put_lens_words(frame_params& frame, const lens_words& words)
	{
		for (int r = 0; r < 4; r++)
			frame.mx[r] = frame.my[r] = frame.k_near[r] = frame.k_far[r] = 0.0f;
		for (int c = 0; c < 3; c++)
			frame.mx[c] = words.u[c], frame.my[c] = words.v[c], frame.k_near[c] = words.fwd[c];
		frame.mx[3] = words.focus;
	}
}

extern "C" rt_hip_status rt_hip_lens_from_spec(const char* spec, rt_hip_lens* out_lens)
{
	const rt_hip::lens_check c = rt_hip::lens_from_spec(spec, out_lens);
	return c.status ? rt_hip::fail(c.status, "%s", c.message) : RT_HIP_OK;
}
