// rt_amd/csrc/lens_rules.hpp — the rules of RT_HIP_FLAG_THIN_LENS, written ONCE so that hipcc and g++ both compile
// them: the lens builds of render_queue (kernels.hip) run this text per restarting lane, tests/native/lens_reference.cpp restates the
// sample loop on the CPU over the very same functions, and the device's frames must equal that restatement bit for bit.
//
// What it holds: the map from the two numerators of one generator step to a point of the unit disk, and the ray through that point of
// the lens that meets the pinhole's ray on the focus plane.  What it does NOT hold: the generator, the pinhole's primary ray and the
// normalisation of the new direction — the callers' — and the leaf functions, which come from whoever includes this header, in
// namespace rt_hip::lens::leaf, BEFORE the inclusion:
//     float divide(float a, float b)     a / b, correctly rounded
// kernels.hip and kat.hip hand in contract.hpp's own, the CPU restatement plain '/': none of them is restated here.
//
// The arithmetic is + - x, fused multiply-adds ONLY where RT_HIP_LENS_FMA is written, one correctly rounded division per function,
// compare-and-select; both compilers are told not to contract (-ffp-contract=off) and every operation stands in ONE order:
//   x = fma(ka, 2^-23, -1), y = fma(kb, 2^-23, -1)                 exact (ka, kb < 2^24)
//   first = |x| > |y|;  major = first ? x : y;  minor = first ? y : x         (a tie takes the second branch)
//   major == 0: the point is (0, 0), by select — the quotient below is then taken over 1, never over 0
//   q = minor / major;  psi = q * float(pi / 4);  z = psi * psi
//   s = psi * fma(fma(fma(fma(S4, z, S3), z, S2), z, S1), z, 1)      S = -1/6, 1/120, -1/5040, 1/362880, each rounded to binary32
//   c =       fma(fma(fma(fma(C4, z, C3), z, C2), z, C1), z, 1)      C = -1/2, 1/24, -1/720, 1/40320
//   first: (lx, ly) = (major * c, major * s);  else (major * s, major * c)
// and, for the pinhole's ray (o, d), the eye E and the ten lens words U, V, fwd, focus (lens.hpp):
//   L_k = fma(U_k, lx, V_k * ly);  cosine = dot(d, fwd);  t = focus / cosine
//   origin_k = E_k + L_k;  toward_k = fma(d_k, t, -L_k)              the caller normalises toward
//   bent = cosine > 0 && |t| <= FLT_MAX                              (false for a NaN): otherwise the ray stays (o, d)
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define RT_HIP_LENS_FN __host__ __device__ __forceinline__
#else
#define RT_HIP_LENS_FN inline
#endif
#define RT_HIP_LENS_FMA(a, b, c) __builtin_fmaf((a), (b), (c))

namespace rt_hip
{
namespace lens
{
	constexpr float quarter_pi = 0x1.921fb6p-1f; // float(pi / 4)
	constexpr float sin_1 = -0x1.555556p-3f, sin_2 = 0x1.111112p-7f, sin_3 = -0x1.a01a02p-13f, sin_4 = 0x1.71de3ap-19f; // -1/6, 1/120, -1/5040, 1/362880
	constexpr float cos_1 = -0x1.0p-1f, cos_2 = 0x1.555556p-5f, cos_3 = -0x1.6c16c2p-10f, cos_4 = 0x1.a01a02p-16f;		// -1/2, 1/24, -1/720, 1/40320
	constexpr float largest_finite = 0x1.fffffep+127f;

	struct disk_point
	{
		float x, y;
	};

	// the concentric map: the numerators (ka, kb) of one generator step to a point of the unit disk, area-preserving
	RT_HIP_LENS_FN disk_point disk(uint32_t ka, uint32_t kb)
	{
		const float x = RT_HIP_LENS_FMA(static_cast<float>(ka), 0x1.0p-23f, -1.0f);
		const float y = RT_HIP_LENS_FMA(static_cast<float>(kb), 0x1.0p-23f, -1.0f);
		const bool first = __builtin_fabsf(x) > __builtin_fabsf(y);
		const float major = first ? x : y;
		const float minor = first ? y : x;
		const bool centre = major == 0.0f;
		const float q = leaf::divide(minor, centre ? 1.0f : major);
		const float psi = q * quarter_pi;
		const float z = psi * psi;
		const float s = psi * RT_HIP_LENS_FMA(RT_HIP_LENS_FMA(RT_HIP_LENS_FMA(RT_HIP_LENS_FMA(sin_4, z, sin_3), z, sin_2), z, sin_1), z, 1.0f);
		const float c = RT_HIP_LENS_FMA(RT_HIP_LENS_FMA(RT_HIP_LENS_FMA(RT_HIP_LENS_FMA(cos_4, z, cos_3), z, cos_2), z, cos_1), z, 1.0f);
		const float along = major * c, across = major * s;
		disk_point p;
		p.x = centre ? 0.0f : (first ? along : across);
		p.y = centre ? 0.0f : (first ? across : along);
		return p;
	}

	// the ten words the kernels are handed (lens.hpp, make_lens_words): U = aperture * right, V = aperture * up, fwd, focus
	template <class V>
	struct words
	{
		V u, v, fwd;
		float focus;
	};

	template <class V>
	struct bent_ray
	{
		V origin, toward; // the point on the lens, and the vector to the focus-plane point: NOT normalised (the caller's normalize)
		bool bent;		  // false: the ray stays the pinhole's
	};

	template <class V>
	RT_HIP_LENS_FN float dot3(V a, V b)
	{
		return RT_HIP_LENS_FMA(a.z, b.z, RT_HIP_LENS_FMA(a.y, b.y, a.x * b.x)); // the contract's dot
	}

	// the lens ray of the pinhole's ray with the NORMALISED direction d, for the eye E and the point p of the unit disk
	template <class V>
	RT_HIP_LENS_FN bent_ray<V> bend(V d, V eye, words<V> w, disk_point p)
	{
		V l;
		l.x = RT_HIP_LENS_FMA(w.u.x, p.x, w.v.x * p.y), l.y = RT_HIP_LENS_FMA(w.u.y, p.x, w.v.y * p.y), l.z = RT_HIP_LENS_FMA(w.u.z, p.x, w.v.z * p.y);
		const float cosine = dot3(d, w.fwd);
		const float t = leaf::divide(w.focus, cosine);
		bent_ray<V> r;
		r.origin.x = eye.x + l.x, r.origin.y = eye.y + l.y, r.origin.z = eye.z + l.z;
		r.toward.x = RT_HIP_LENS_FMA(d.x, t, -l.x), r.toward.y = RT_HIP_LENS_FMA(d.y, t, -l.y), r.toward.z = RT_HIP_LENS_FMA(d.z, t, -l.z);
		r.bent = cosine > 0.0f && __builtin_fabsf(t) <= largest_finite;
		return r;
	}
}
}
