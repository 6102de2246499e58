// rt_amd/csrc/sky_band.cpp — the sky band's rule (sky_band.hpp): host-only, plain C++17.
//
// In the kernels' own terms.  The primary ray of pixel (x, y) with jitter numerators (ka, kb) starts at eye + T and runs along T,
//   T = d0 + d1 u + d2 v,   u = x + ka 2^-24,  v = y + kb 2^-24      (frame_params::ray_d0 / ray_d1 / ray_d2, ray_j = ray_d 2^-24)
// affine in the continuous pixel position.  For a sphere (c, r^2) with w = c - eye, probe_sphere / finish_sphere (scan.hpp) compute
//   e = w - T,   a = e . T^,   disc = r^2 - (|e|^2 - a^2),   t = a - f  where |e|^2 >= r^2   (f = sqrt(disc) >= 0)
// and with q = w . T (affine too):  |e|^2 - a^2 = |w|^2 - q^2 / |T|^2  (the squared distance of c from the ray's line) and
// a = (q - |T|^2) / |T|.  Over a cell of rays — a rectangle of (u, v) — the sphere is certainly missed if
//   (A) the line misses with room:  |w|^2 - max(q^2) / min|T|^2 - r^2 >= eps S  (or (A'): the same with the cell's exact
//       max(q^2 / |T|^2), found on its edges), or
//   (B) the origin is outside and the centre behind every ray:  min|e|^2 - r^2 >= eps S  and  max(q) - min|T|^2 <= -eps L max|T|
// with the scales S = |w|^2 + r^2 + max|T|^2 + m^2 / 64 and L = |w| + max|T| + m / 8, m = |eye| + |c| (the terms in m cover the
// rounding of eye + T and c - (eye + T), which is relative to the points' distance from the world's origin, not to |w|).  q is
// affine: its extremes sit at the cell's corners; |T|^2 is a convex quadratic: its maximum sits at a corner, its minimum is worked
// out exactly; |e|^2 = |w|^2 - 2 q + |T|^2 >= |w|^2 - 2 max(q) + min|T|^2.  The cell is taken one pixel larger on every side: that
// covers the binary32 evaluation of T (2^-22 of its length, against a pixel step of at least 2^-17 of it).
#include "sky_band.hpp"

#include <cmath>
#include <initializer_list>

namespace rt_hip
{
	namespace
	{
		struct ray_field // T(u, v) = d0 + d1 u + d2 v and the Gram matrix of |T|^2
		{
			double d0[3], d1[3], d2[3];
			double g00, g01, g02, g11, g12, g22;
			double det, inv_det, inv_g11, inv_g22; // (the reciprocals: least_length2 runs a few hundred times per frame)
		};

		double length2_at(const ray_field& f, double u, double v)
		{
			return f.g00 + u * (2.0 * f.g01 + u * f.g11) + v * (2.0 * f.g02 + v * f.g22) + 2.0 * u * v * f.g12;
		}

		// (every value here is finite — sky_band_rows has looked — so these are fmin and fmax, inlined)
		double lesser(double a, double b) { return b < a ? b : a; }
		double greater(double a, double b) { return b > a ? b : a; }
		double clamp_to(double x, double lo, double hi) { return x < lo ? lo : (x > hi ? hi : x); }

		// the minimum of |T|^2 over [u0, u1] x [v0, v1]: a convex quadratic — the free minimum if it lies inside, else the least of
		// the four edges' minima
		double least_length2(const ray_field& f, double u0, double u1, double v0, double v1)
		{
			const double u = (f.g12 * f.g02 - f.g22 * f.g01) * f.inv_det, v = (f.g12 * f.g01 - f.g11 * f.g02) * f.inv_det;
			if (u >= u0 && u <= u1 && v >= v0 && v <= v1)
				return length2_at(f, u, v);
			double least = INFINITY;
			for (const double fixed_u : { u0, u1 })
				least = lesser(least, length2_at(f, fixed_u, clamp_to(-(f.g02 + fixed_u * f.g12) * f.inv_g22, v0, v1)));
			for (const double fixed_v : { v0, v1 })
				least = lesser(least, length2_at(f, clamp_to(-(f.g01 + fixed_v * f.g12) * f.inv_g11, u0, u1), fixed_v));
			return least;
		}

		struct sphere_terms
		{
			double q0, q1, q2; // q(u, v) = w . T
			double w2, r2, m;  // |w|^2, r^2, |eye| + |c|
			double w_length;   // |w|
			bool pierces;	   // the line through the eye along w meets the near plane: at (u_pierce, v_pierce)
			double u_pierce, v_pierce;
		};

		// is the sphere certainly missed by every ray of pixel columns [x0, x1), rows [y0, y1)?
		bool certainly_missed(const ray_field& f, const sphere_terms& s, uint32_t x0, uint32_t x1, uint32_t y0, uint32_t y1)
		{
			const double u0 = static_cast<double>(x0) - 1.0, u1 = static_cast<double>(x1) + 1.0, v0 = static_cast<double>(y0) - 1.0, v1 = static_cast<double>(y1) + 1.0;
			double q_min = INFINITY, q_max = -INFINITY, t2_max = 0.0, t2_corner[4];
			for (int corner = 0; corner < 4; corner++)
			{
				const double u = (corner & 1) ? u1 : u0, v = (corner & 2) ? v1 : v0;
				const double q = s.q0 + s.q1 * u + s.q2 * v;
				q_min = lesser(q_min, q), q_max = greater(q_max, q);
				t2_corner[corner] = length2_at(f, u, v);
				t2_max = greater(t2_max, t2_corner[corner]);
			}
			const double t2_min = least_length2(f, u0, u1, v0, v1);
			if (!(t2_min > 0.0)) // (a NaN fails too)
				return false;
			const double scale = s.w2 + s.r2 + t2_max + s.m * s.m * (1.0 / 64.0);
			const double room = sky_band_epsilon * scale;
			const double q2_max = greater(q_min * q_min, q_max * q_max);
			if (s.w2 - q2_max / t2_min - s.r2 >= room) // (A)
				return true;
			const double t_max = std::sqrt(t2_max);
			const double behind = sky_band_epsilon * (s.w_length + t_max + s.m * 0.125) * t_max;
			if (s.w2 - 2.0 * q_max + t2_min - s.r2 >= room && q_max - t2_min <= -behind) // (B)
				return true;
			// (A') the same condition with the EXACT largest q^2 / |T|^2 of the cell, where (A) pairs the largest q with the least |T| of
			// different rays.  On the near plane q^2 / |T|^2 has no stationary point but its zeros (q = 0) and the point where w's own
			// line pierces the plane: its gradient q (2 |T|^2 grad q - q grad |T|^2) / |T|^4 vanishes beside q = 0 only where
			// |T|^2 w - q T is normal to the plane, and that vector is normal to T, which never lies in the plane.  So with the
			// piercing point outside the cell the maximum sits on an edge; along an edge q is linear and |T|^2 quadratic in the
			// running coordinate, and the ratio's derivative has ONE root beside q = 0: the ends and that root are all there is.
			if (s.pierces && s.u_pierce >= u0 && s.u_pierce <= u1 && s.v_pierce >= v0 && s.v_pierce <= v1)
				return false;
			double ratio_max = q2_max / t2_max; // (any ray's ratio bounds the maximum from below: the corners' come for free)
			for (int corner = 0; corner < 4; corner++)
			{
				const double u = (corner & 1) ? u1 : u0, v = (corner & 2) ? v1 : v0;
				const double q = s.q0 + s.q1 * u + s.q2 * v;
				ratio_max = greater(ratio_max, q * q / t2_corner[corner]);
			}
			for (int edge = 0; edge < 4; edge++)
			{
				// |T|^2 = a + 2 b t + c t^2 and q = k0 + k1 t along the edge; edges 0, 1: u fixed, t = v; edges 2, 3: v fixed, t = u
				const bool along_v = edge < 2;
				const double fixed = along_v ? (edge ? u1 : u0) : (edge == 3 ? v1 : v0);
				const double t0 = along_v ? v0 : u0, t1 = along_v ? v1 : u1;
				const double a = along_v ? f.g00 + fixed * (2.0 * f.g01 + fixed * f.g11) : f.g00 + fixed * (2.0 * f.g02 + fixed * f.g22);
				const double b = along_v ? f.g02 + fixed * f.g12 : f.g01 + fixed * f.g12;
				const double c = along_v ? f.g22 : f.g11;
				const double k0 = along_v ? s.q0 + s.q1 * fixed : s.q0 + s.q2 * fixed, k1 = along_v ? s.q2 : s.q1;
				const double den = k1 * b - k0 * c;
				if (den != 0.0)
				{
					const double t = -(k1 * a - k0 * b) / den;
					if (t > t0 && t < t1)
					{
						const double q = k0 + k1 * t;
						ratio_max = greater(ratio_max, q * q / (a + t * (2.0 * b + t * c)));
					}
				}
			}
			return s.w2 - ratio_max - s.r2 >= room;
		}

		// Within one strip: is the sphere certainly missed in all of columns [x0, x1), rows [y0, y1)?  A cell that cannot be shown at once
		// is cut in two, its rows or its columns, down to single rows of sky_band_cell_columns columns.  (Rows within a strip matter: of
		// a ground sphere under a level camera (B) holds down to a hair above the horizontal and (A) from a few rows above it — a cell that
		// spans more than their overlap shows neither.)
		bool strip_is_clear(const ray_field& f, const sphere_terms& s, uint32_t x0, uint32_t x1, uint32_t y0, uint32_t y1, bool asked = false)
		{
			if (!asked && certainly_missed(f, s, x0, x1, y0, y1)) // (asked: the caller has, in vain)
				return true;
			const uint32_t columns = x1 - x0, rows = y1 - y0;
			const bool narrow = columns <= sky_band_cell_columns;
			if (rows > 1u && (narrow || rows * 32u >= columns))
			{
				const uint32_t middle = y0 + rows / 2u;
				return strip_is_clear(f, s, x0, x1, middle, y1) && strip_is_clear(f, s, x0, x1, y0, middle); // (the lower half first: the likelier to fail)
			}
			if (narrow)
				return false;
			const uint32_t middle = x0 + columns / 2u;
			return strip_is_clear(f, s, x0, middle, y0, y1) && strip_is_clear(f, s, middle, x1, y0, y1);
		}

		// The first row y of [y0, y1] (in whole strips from y0) such that the sphere is certainly missed in rows [y0, y) of columns [x0, x1);
		// y1: in all of them.  A cell of several strips that cannot be shown at once is cut in two — its rows while it is not much wider than
		// tall, else its columns — and the second half is asked only for what the first left.
		uint32_t first_doubtful_row(const ray_field& f, const sphere_terms& s, uint32_t x0, uint32_t x1, uint32_t y0, uint32_t y1)
		{
			if (y0 >= y1 || certainly_missed(f, s, x0, x1, y0, y1))
				return y1;
			const uint32_t columns = x1 - x0, strips = (y1 - y0) / sky_band_strip_rows;
			if (strips <= 1u)
				return strip_is_clear(f, s, x0, x1, y0, y1, true) ? y1 : y0;
			if (columns <= sky_band_cell_columns || (y1 - y0) * 4u >= columns)
			{
				const uint32_t middle = y0 + (strips / 2u) * sky_band_strip_rows;
				const uint32_t upper = first_doubtful_row(f, s, x0, x1, y0, middle);
				return upper < middle ? upper : first_doubtful_row(f, s, x0, x1, middle, y1);
			}
			const uint32_t middle = x0 + columns / 2u;
			const uint32_t left = first_doubtful_row(f, s, x0, middle, y0, y1);
			return left == y0 ? y0 : first_doubtful_row(f, s, middle, x1, y0, left);
		}
	}

	uint32_t sky_band_rows(const sky_band_request& request)
	{
		if (!request.frame || request.pass || request.adaptive || (request.flags & sky_band_excluded_flags) || request.n_planes != 0u)
			return 0u;
		if (!(request.scan > 0 || request.scan == scan_resident) || request.n_spheres > sky_band_max_spheres || (request.n_spheres && !request.spheres))
			return 0u;
		const frame_params& p = *request.frame;
		// a one-shot frame of the whole image through the pinhole form
		if (p.world != 1u || p.rank != 0u || p.local_rows != p.height || !p.pinhole)
			return 0u;
		if (!p.width || p.width > sky_band_max_side || p.height > sky_band_max_side || p.height < sky_band_strip_rows)
			return 0u;
		// (a frame without samples or without a primary segment has no sky to add; beyond 2^20 samples the windows alias)
		if (!p.samples_per_pixel || p.samples_per_pixel >= (1u << 20) || !p.max_bounces)
			return 0u;

		ray_field f{};
		double eye[3], eye2 = 0.0;
		for (int c = 0; c < 3; c++)
		{
			f.d0[c] = p.ray_d0[c], f.d1[c] = p.ray_d1[c], f.d2[c] = p.ray_d2[c];
			eye[c] = p.ray_eye[c];
			eye2 += eye[c] * eye[c];
			// (the kernels' per-sample steps are the per-pixel ones scaled exactly: a subnormal step would not be)
			if (!(static_cast<double>(p.ray_j1[c]) * 0x1.0p24 == f.d1[c]) || !(static_cast<double>(p.ray_j2[c]) * 0x1.0p24 == f.d2[c]))
				return 0u;
			f.g00 += f.d0[c] * f.d0[c], f.g01 += f.d0[c] * f.d1[c], f.g02 += f.d0[c] * f.d2[c];
			f.g11 += f.d1[c] * f.d1[c], f.g12 += f.d1[c] * f.d2[c], f.g22 += f.d2[c] * f.d2[c];
		}
		f.det = f.g11 * f.g22 - f.g12 * f.g12;
		f.inv_det = 1.0 / f.det, f.inv_g11 = 1.0 / f.g11, f.inv_g22 = 1.0 / f.g22;
		// (every comparison fails for a NaN; an infinite constant makes g00 or the determinant infinite or NaN)
		if (!(f.g00 < INFINITY) || !(eye2 < INFINITY) || !(f.g11 > 0.0) || !(f.g22 > 0.0) || !(f.det > 0x1.0p-20 * f.g11 * f.g22) || !(f.det < INFINITY))
			return 0u;

		uint32_t rows = (p.height / sky_band_strip_rows) * sky_band_strip_rows;
		for (uint32_t i = 0; i < request.n_spheres && rows; i++)
		{
			const float* const sphere = request.spheres + 4u * static_cast<size_t>(i);
			sphere_terms s{};
			double c2 = 0.0;
			for (int c = 0; c < 3; c++)
			{
				const double centre = sphere[c], w = centre - eye[c];
				c2 += centre * centre;
				s.w2 += w * w;
				s.q0 += w * f.d0[c], s.q1 += w * f.d1[c], s.q2 += w * f.d2[c];
			}
			s.r2 = sphere[3];
			s.m = std::sqrt(eye2) + std::sqrt(c2);
			s.w_length = std::sqrt(s.w2);
			// where lambda w = d0 + u d1 + v d2: lambda from the plane's normal n = d1 x d2, then (u, v) through the Gram matrix
			const double n[3] = { f.d1[1] * f.d2[2] - f.d1[2] * f.d2[1], f.d1[2] * f.d2[0] - f.d1[0] * f.d2[2], f.d1[0] * f.d2[1] - f.d1[1] * f.d2[0] };
			double wn = 0.0, d0n = 0.0;
			for (int c = 0; c < 3; c++)
				wn += (static_cast<double>(sphere[c]) - eye[c]) * n[c], d0n += f.d0[c] * n[c];
			s.pierces = false;
			if (wn != 0.0)
			{
				const double lambda = d0n / wn, right1 = lambda * s.q1 - f.g01, right2 = lambda * s.q2 - f.g02;
				s.u_pierce = (f.g22 * right1 - f.g12 * right2) * f.inv_det, s.v_pierce = (f.g11 * right2 - f.g12 * right1) * f.inv_det;
				s.pierces = true;
				if (!(s.u_pierce > -INFINITY && s.u_pierce < INFINITY && s.v_pierce > -INFINITY && s.v_pierce < INFINITY)) // (an overflow: as good as parallel, but say "inside" to be safe)
					return 0u;
			}
			if (!(c2 < INFINITY) || !(s.w2 < INFINITY) || !(s.r2 >= 0.0) || !(s.r2 < INFINITY))
				return 0u;
			rows = first_doubtful_row(f, s, 0u, p.width, 0u, rows);
		}
		return rows;
	}
}
