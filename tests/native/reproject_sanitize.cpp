// tests/native/reproject_sanitize.cpp — `make sanitize-temporal`: the host-only unit of temporal accumulation (rt_amd/csrc/temporal.cpp)
// and the CPU restatement's serial loop over rt_amd/csrc/reproject_rules.hpp behind a main() of their own, for AddressSanitizer and
// UndefinedBehaviorSanitizer.  TEST INFRASTRUCTURE: CPU only, never loaded into python, never near a GPU.
//
// The case: a 70 x 41 frame of two spheres over a floor, three frames chained — the camera steps sideways far enough that projections
// leave the frame on one side, then turns by half a turn so that every point projects from behind the previous camera — with a NaN
// and an infinity planted in the history; a singular and a non-finite matrix; every parameter refusal.  It checks only what the
// rules promise about such inputs (no pixel reads outside its arrays — the sanitizers' business — and nothing non-finite spreads).
#include "reproject_reference.cpp"

#include <cmath>
#include <cstdlib>
#include <vector>

namespace
{
	constexpr uint32_t W = 70, H = 41;

	int failures = 0;
	void expect(bool ok, const char* what)
	{
		if (!ok)
		{
			std::fprintf(stderr, "FAILED: %s\n", what);
			failures++;
		}
	}

	// A pinhole camera at the eye looking along -z (turned: +z), clip -> world, [r * 4 + c]: the clip point (x, y, z) is the world point
	// eye + (s half_w x, half_h y, -s) / (2 - z) — a third of the way to the plane one unit ahead at z = -1, on it at z = 1.
	void camera(float ex, float ey, float ez, bool turned, float* m)
	{
		const float s = turned ? -1.0f : 1.0f, half_w = 0.8f, half_h = 0.8f * H / W;
		const float rows[16] = { s * half_w, 0, -ex, 2 * ex, 0, half_h, -ey, 2 * ey, 0, 0, -ez, 2 * ez - s, 0, 0, -1, 2 };
		for (int i = 0; i < 16; i++)
			m[i] = rows[i];
	}
}

int main()
{
	// the scene: columns as rt_hip_scene wants them
	const float cx[] = { 0.0f, 1.2f, 0.3f }, cy[] = { 0.5f, 0.4f, 0.6f }, cz[] = { 0.0f, -0.5f, 6.0f }, radius[] = { 0.5f, 0.4f, 0.6f };
	const uint32_t sphere_material[] = { 0, 1, 0 };
	const float nx[] = { 0.0f }, ny[] = { 1.0f }, nz[] = { 0.0f }, d[] = { 0.0f };
	const uint32_t plane_material[] = { 1 };
	const uint32_t material_type[] = { 0, 0 };
	const float albedo[] = { 0.8f, 0.2f, 0.2f, 1.0f, 0.5f, 0.5f, 0.5f, 1.0f }, roughness[] = { 0.0f, 0.0f }, reflectivity[] = { 1.0f, 1.0f };
	rt_hip_scene scene{};
	scene.n_spheres = 3, scene.sphere_center_x = cx, scene.sphere_center_y = cy, scene.sphere_center_z = cz, scene.sphere_radius = radius, scene.sphere_material = sphere_material;
	scene.n_planes = 1, scene.plane_normal_x = nx, scene.plane_normal_y = ny, scene.plane_normal_z = nz, scene.plane_d = d, scene.plane_material = plane_material;
	scene.n_materials = 2, scene.material_type = material_type, scene.material_albedo = albedo, scene.material_roughness = roughness, scene.material_reflectivity = reflectivity;
	scene.samples_per_pixel = 16, scene.max_bounces = 4;

	const size_t pixels = static_cast<size_t>(W) * H;
	struct frame
	{
		float matrix[16];
		std::vector<float> guide, rgb, out, record;
		uint32_t found = 0;
	};
	const struct
	{
		float x, y, z;
		bool turned;
	} poses[3] = { { 0.0f, 1.0f, 3.0f, false }, { 1.9f, 1.0f, 3.0f, false }, { 1.9f, 1.0f, 3.0f, true } };
	frame frames[3];
	for (int f = 0; f < 3; f++)
	{
		frame& fr = frames[f];
		camera(poses[f].x, poses[f].y, poses[f].z, poses[f].turned, fr.matrix);
		float forward[16];
		expect(forward_view_projection(fr.matrix, forward).status == RT_HIP_OK, "the test's own camera is invertible");
		std::memcpy(scene.inverse_view_projection, fr.matrix, sizeof fr.matrix);
		fr.guide.assign(pixels * 8, 0.0f), fr.rgb.assign(pixels * 3, 0.0f), fr.out.assign(pixels * 3, -1.0f), fr.record.assign(pixels * 8, -1.0f);
		// the guide, composed as tests/denoise_reference.py composes it: the oracle's centre ray and its closest hit
		std::vector<float> origins(pixels * 3), directions(pixels * 3), distance(pixels), normal(pixels * 3);
		std::vector<uint32_t> kind(pixels), index(pixels);
		for (uint32_t y = 0; y < H; y++)
			for (uint32_t x = 0; x < W; x++)
				oracle_primary_ray(&scene, W, H, x, y, 0x1.0p23f, 0x1.0p23f, &origins[(y * W + x) * 3], &directions[(y * W + x) * 3]);
		oracle_closest_hit(&scene, static_cast<uint32_t>(pixels), origins.data(), directions.data(), distance.data(), kind.data(), index.data(), normal.data());
		size_t hits = 0;
		for (size_t i = 0; i < pixels; i++)
		{
			const uint32_t id = kind[i] ? 1u + (kind[i] == 1u ? index[i] : scene.n_spheres + index[i]) : 0u;
			float* const g = &fr.guide[i * 8];
			g[0] = normal[i * 3], g[1] = normal[i * 3 + 1], g[2] = normal[i * 3 + 2], g[3] = kind[i] ? distance[i] : -1.0f;
			std::memcpy(g + 7, &id, sizeof id);
			hits += kind[i] ? 1u : 0u;
			for (int c = 0; c < 3; c++)
				fr.rgb[i * 3 + c] = static_cast<float>((i * 7 + c * 3 + f) % 11) / 10.0f;
		}
		expect(hits > pixels / 8 && hits < pixels, "the frame shows hits and sky");
		frame* const before = f ? &frames[f - 1] : nullptr;
		if (before) // poison the history: it must not spread
		{
			before->out[(20 * W + 30) * 3 + 1] = NAN;
			before->out[(30 * W + 5) * 3] = INFINITY;
		}
		const int status = reproject_ref_frame(&scene, W, H, before ? before->matrix : nullptr, fr.guide.data(), fr.rgb.data(), 16, before ? before->out.data() : nullptr, before ? before->record.data() : nullptr, nullptr, fr.out.data(),
											   fr.record.data(), &fr.found);
		expect(status == RT_HIP_OK, "the step is accepted");
		bool finite = true;
		for (const float v : fr.out)
			finite = finite && std::isfinite(v);
		expect(finite, "nothing non-finite comes out of a finite frame");
		std::printf("frame %d: %u of %zu pixels found history (%zu hits)\n", f, fr.found, pixels, hits);
	}
	expect(frames[0].found == 0, "no history, no pixel with history");
	expect(frames[1].found > 0 && frames[1].found < pixels, "a sideways step keeps part of the history and loses the part that left the frame");
	expect(frames[2].found == 0, "after half a turn nothing is found: what was seen lies behind the camera");

	// the host unit's refusals
	float singular[16] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1 }, out[16];
	expect(forward_view_projection(singular, out).status == RT_HIP_INVALID_ARGUMENT, "a singular matrix is refused");
	singular[5] = NAN;
	expect(forward_view_projection(singular, out).status == RT_HIP_INVALID_ARGUMENT, "a NaN matrix is refused");
	expect(reproject_ref_frame(&scene, W, H, singular, frames[2].guide.data(), frames[2].rgb.data(), 16, frames[1].out.data(), frames[1].record.data(), nullptr, frames[2].out.data(), frames[2].record.data(), nullptr) == RT_HIP_INVALID_ARGUMENT,
		   "... by the step too");
	rt_hip_temporal_params p = default_temporal_params();
	expect(check_temporal_params(p).status == RT_HIP_OK, "the defaults pass");
	p.max_history_samples = 0;
	expect(check_temporal_params(p).status == RT_HIP_INVALID_ARGUMENT, "max_history_samples = 0 is refused");
	p = default_temporal_params(), p.position_tolerance = -1.0f;
	expect(check_temporal_params(p).status == RT_HIP_INVALID_ARGUMENT, "a negative position_tolerance is refused");
	p = default_temporal_params(), p.normal_threshold = NAN;
	expect(check_temporal_params(p).status == RT_HIP_INVALID_ARGUMENT, "a NaN normal_threshold is refused");
	frame_key a{}, b{};
	expect(same_history(a, b), "equal keys are one history");
	b.width = 1;
	expect(!same_history(a, b), "another size starts again");

	std::printf(failures ? "%d check(s) FAILED\n" : "all checks passed\n", failures);
	return failures ? 1 : 0;
}
