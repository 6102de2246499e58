// rt_amd/host/main.cpp — rt_headless: a windowless driver for rt renderers.
//
// The reference's only driver is an SDL window (src/main.cpp, src/window.cpp): no headless mode, and no flags for
// frame size, samples, seed or an output file.  This driver keeps the reference's CLI where it has
// one — `--list`, `--scene <path>` (default: first *.toml found), `--renderer <name>` with prefix matching, the
// same log lines (src/main.cpp:30-47,68-81,97-99,335-351) — and adds what a benchmark needs:
//   --size WxH   frame size (the reference uses the window size, 800x600 initially: src/main.cpp:153)
//   --spp N / --bounces N   override the scene file's values
//   --seed N     pin the random streams (exported to the renderer as RT_HIP_SEED)
//   --frames N   render N frames, report the last
//   --out file.ppm   write the frame (binary PPM, RGB)
//   --progressive SAMPLES   the frame in passes of SAMPLES samples per pixel (exported to the renderer as RT_HIP_PROGRESSIVE):
//                render() is called ceil(spp / SAMPLES) times — every call shows the frame as it stands — and the last frame,
//                the same as without the option, is the one reported and written (hip renderers only; not together with --frames)
//   --denoise               with --progressive (or --temporal or --upscale, see there): every pass's frame goes through the guide-buffer denoiser (exported to the renderer as
//                           RT_HIP_DENOISE=always: rt_hip_denoise_progressive after every pass, the last one included), so the frame
//                           written is the denoised frame of the last pass
//   --boxes                 the traced frame hits the scene's boxes too (exported to the renderer as RT_HIP_TRACE_BOXES=1: RT_HIP_FLAG_TRACE_BOXES);
//                           hip renderers only, not with --progressive
//   --box-bvh               with --boxes: the boxes are reached through a hierarchy of their own, any number of them, the same frame bit for
//                           bit (exported to the renderer as RT_HIP_BOX_BVH=1: RT_HIP_FLAG_BOX_BVH); implies nothing on its own and is
//                           refused without --boxes, and with --temporal
//   --temporal              every frame is one frame of temporal accumulation (exported to the renderer as RT_HIP_TEMPORAL=1:
//                           rt_hip_render_temporal): traced whole with a seed of its own and blended with the history kept across camera
//                           moves; with --denoise the blended frame goes through the a-trous filter too.  Hip renderers only, not with
//                           --progressive; with --frames N the last frame is the one written
//   --adaptive THRESHOLD    adaptive sampling (exported to the renderer as RT_HIP_ADAPTIVE=THRESHOLD: rt_hip_render_adaptive): passes of
//                           16 samples — or of --progressive SAMPLES — over the pixels that have not converged yet; render() is called
//                           until the accumulation is complete, the last frame is written, and the samples traced are printed against
//                           pixels x spp.  Hip renderers only; not with --frames, --temporal, --boxes or --denoise
//   --upscale FACTOR        2, 3 or 4: every frame is traced at ceil(size / FACTOR) and rebuilt at full size by the guided upsampler (exported
//                           to the renderer as RT_HIP_UPSCALE=FACTOR: rt_hip_render_upscaled); with --denoise the traced low
//                           frame goes through the a-trous filter first.  Hip renderers only; not with --progressive, --temporal,
//                           --adaptive, --light or --box-bvh
//   --light KEY=R,G,B       repeatable: the materials named KEY (or the material of that index) are LIGHTS of that emission; KEY=V is a grey
//                           light (exported to the renderer as RT_HIP_LIGHTS, the items joined with ';': rt_hip_lights_from_spec,
//                           rt_hip_set_emission, RT_HIP_FLAG_EMISSION).  Hip renderers only; not with --progressive, --adaptive,
//                           --temporal, --denoise or --boxes
//   --direct-light          with --light: lambert surfaces sample the sphere lights directly (exported as RT_HIP_DIRECT_LIGHT=1:
//                           RT_HIP_FLAG_DIRECT_LIGHT).  Not without --light, and not where --light is refused
//   --tonemap CURVE[:EXPOSURE]   every frame is exposed and tone-mapped on the device before it is packed (exported to the renderer as
//                           RT_HIP_TONEMAP: rt_hip_render_tonemapped): CURVE is none, reinhard or aces, EXPOSURE auto (metered
//                           from the frame, the default) or a positive number.  What --light makes bright is the point.  Hip tracers only,
//                           one-shot frames only: not with --progressive, --temporal, --adaptive or --upscale
//   --bloom SPEC            every frame gets the glow of what is brighter than the display, on the device, in front of the tone curve (exported to
//                           the renderer as RT_HIP_BLOOM: rt_hip_render_bloomed): SPEC is default, or KEY=VALUE items separated
//                           by ',' with the keys intensity, threshold, knee, scatter and levels.  With --tonemap that curve follows; alone the
//                           finish is none:1, the plain square root.  Refused where --tonemap is
//   --lens aperture=A,focus=F   every frame is taken through a thin lens of radius A that is sharp at distance F along the view direction
//                           (exported to the renderer as RT_HIP_LENS: rt_hip_set_lens and RT_HIP_FLAG_THIN_LENS).  One-shot
//                           frames of a hip renderer only: not with --progressive, --adaptive, --temporal, --denoise, --upscale, --boxes or
//                           --light; it composes with --tonemap and --bloom
//   --dolly DX,DY,DZ        the camera moves by that much in world space before every frame after the first (camera::pose)
//   --shared-frame NAME --rank R --world N   this process is rank R of N rt_headless processes that render ONE frame
//                together (one per GPU: RT_HIP_DEVICE picks this one's): the back buffer is every process's mapping of the
//                POSIX shared-memory object /NAME_frame (rank 0 creates it) and the plug-in joins the frame group
//                /NAME_group (RT_HIP_GROUP, rt_hip_join_frame_group).  Rank 0 clears the buffer and writes --out.
// It renders through renderer_interface::render exactly as window::loop does (src/window.cpp:213-217 via
// src/main.cpp:315-321): clear to opaque black, then render(scene, pixels, threads).
#include "renderer.hpp"
#include "../../include/rt_hip.h" // (rt_hip_adaptive_last_info, rt_hip_live_frame_locks: what --adaptive asks the module itself; rt_hip_tonemap_from_spec, rt_hip_bloom_from_spec)

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <filesystem>
#include <fstream>
#include <iostream>
#include <memory>
#include <string>

using namespace rt;
using namespace std::string_view_literals;

namespace
{
	// the do-nothing renderer of the reference (src/renderers/null_renderer.cpp): the minimal shape of a plug-in, and a
	// second registry entry for --list / --renderer
	struct null_renderer final : renderer_interface
	{
		void render(const rt::scene&, image_view&, muu::thread_pool&) noexcept override {}
	};
	REGISTER_RENDERER(null_renderer);

	template <typename... Args>
	void log(Args&&... args)
	{
		(std::cout << ... << args) << "\n";
	}

	template <typename... Args>
	void error(Args&&... args)
	{
		std::cerr << "error: ";
		(std::cerr << ... << args) << "\n";
	}

	// reference src/main.cpp:68-81
	const renderers::description* find_renderer_by_name_fuzzy(std::string_view name) noexcept
	{
		if (name.empty())
			return {};
		if (auto desc = renderers::find_by_name(name))
			return desc;
		for (auto& r : renderers::all())
			if (r.name.starts_with(name))
				return &r;
		return {};
	}

	// every rank's mapping of the one shared back buffer: rank 0 creates and sizes the object, the others wait for it
	uint32_t* map_shared_frame(const std::string& name, unsigned rank, size_t bytes)
	{
		int fd = -1;
		for (int attempt = 0; attempt < 600 && fd < 0; attempt++) // (up to a minute for rank 0 to get there)
		{
			fd = rank == 0 ? shm_open(name.c_str(), O_CREAT | O_RDWR, 0600) : shm_open(name.c_str(), O_RDWR, 0600);
			struct stat st;
			if (fd >= 0 && rank != 0 && (fstat(fd, &st) != 0 || static_cast<size_t>(st.st_size) < bytes))
			{
				close(fd);
				fd = -1;
			}
			if (fd < 0)
			{
				if (rank == 0)
					return nullptr;
				usleep(100000);
			}
		}
		if (fd < 0 || (rank == 0 && ftruncate(fd, static_cast<off_t>(bytes)) != 0))
			return nullptr;
		void* const mapping = mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
		close(fd);
		return mapping == MAP_FAILED ? nullptr : static_cast<uint32_t*>(mapping);
	}

	bool write_ppm(const std::string& path, const image_view& img)
	{
		std::ofstream out{ path, std::ios::binary };
		if (!out)
			return false;
		out << "P6\n" << img.size().x << " " << img.size().y << "\n255\n";
		const size_t n = static_cast<size_t>(img.size().x) * img.size().y;
		std::string rgb(n * 3, '\0');
		for (size_t i = 0; i < n; i++)
		{
			const uint32_t p = img.data()[i]; // RGBA8888, reference src/colour.hpp:105
			rgb[i * 3 + 0] = static_cast<char>(p >> 24);
			rgb[i * 3 + 1] = static_cast<char>(p >> 16);
			rgb[i * 3 + 2] = static_cast<char>(p >> 8);
		}
		out.write(rgb.data(), static_cast<std::streamsize>(rgb.size()));
		return static_cast<bool>(out);
	}
}

int main(int argc, char** argv)
{
	std::string scene_path, renderer_name, out_path, shared_name, lights, tonemap, bloom, lens;
	bool direct_light = false;
	unsigned width = 800, height = 600, spp = 0, bounces = 0, frames = 1, rank = 0, world = 1, progressive = 0;
	bool frames_given = false;
	bool list = false;
	bool boxes = false, box_bvh = false, denoise = false, temporal = false, dolly = false, adaptive = false;
	unsigned upscale = 0;
	float dolly_by[3] = { 0.0f, 0.0f, 0.0f };
	// default renderer: the first whose name starts with "hip", else the first registered (reference: first "mg", :350)
	for (auto& r : renderers::all())
		if (renderer_name.empty() && r.name.starts_with("hip"))
			renderer_name = r.name;
	if (renderer_name.empty() && !renderers::all().empty())
		renderer_name = renderers::all().front().name;

	for (int i = 1; i < argc; i++)
	{
		const std::string_view arg = argv[i];
		const auto value = [&]() -> const char*
		{
			if (i + 1 >= argc)
			{
				error("missing value for ", arg);
				std::exit(2);
			}
			return argv[++i];
		};
		if (arg == "--list"sv)
			list = true;
		else if (arg == "--scene"sv)
			scene_path = value();
		else if (arg == "--renderer"sv)
			renderer_name = value();
		else if (arg == "--size"sv)
		{
			if (std::sscanf(value(), "%ux%u", &width, &height) != 2 || !width || !height)
			{
				error("--size expects WxH");
				return 2;
			}
		}
		else if (arg == "--spp"sv)
			spp = static_cast<unsigned>(std::strtoul(value(), nullptr, 10));
		else if (arg == "--bounces"sv)
			bounces = static_cast<unsigned>(std::strtoul(value(), nullptr, 10));
		else if (arg == "--frames"sv)
			frames = static_cast<unsigned>(std::strtoul(value(), nullptr, 10)), frames_given = true;
		else if (arg == "--seed"sv)
			::setenv("RT_HIP_SEED", value(), 1);
		else if (arg == "--out"sv)
			out_path = value();
		else if (arg == "--progressive"sv)
		{
			const char* const samples = value();
			progressive = static_cast<unsigned>(std::strtoul(samples, nullptr, 10));
			if (!progressive)
			{
				error("--progressive expects the samples per pass (>= 1)");
				return 2;
			}
			::setenv("RT_HIP_PROGRESSIVE", std::to_string(progressive).c_str(), 1); // (the number as read here, whatever way it was spelled)
		}
		else if (arg == "--denoise"sv)
		{
			denoise = true;
			::setenv("RT_HIP_DENOISE", "always", 1); // (read by the plug-in: rt_hip_denoise_progressive after every pass, the finished frame too)
		}
		else if (arg == "--boxes"sv)
		{
			boxes = true;
			::setenv("RT_HIP_TRACE_BOXES", "1", 1); // (read by the plug-in: RT_HIP_FLAG_TRACE_BOXES, the traced frame hits the scene's boxes)
		}
		else if (arg == "--box-bvh"sv)
		{
			box_bvh = true;
			::setenv("RT_HIP_BOX_BVH", "1", 1); // (read by the plug-in: RT_HIP_FLAG_BOX_BVH, the boxes through their own hierarchy)
		}
		else if (arg == "--temporal"sv)
		{
			temporal = true;
			::setenv("RT_HIP_TEMPORAL", "1", 1); // (read by the plug-in: every render() is one rt_hip_render_temporal frame)
		}
		else if (arg == "--upscale"sv)
		{
			const char* const factor = value();
			char* end = nullptr;
			const unsigned long parsed = std::strtoul(factor, &end, 10);
			if (end == factor || *end || parsed < 2ul || parsed > 4ul)
			{
				error("--upscale expects the factor (2, 3 or 4)");
				return 2;
			}
			upscale = static_cast<unsigned>(parsed);
			::setenv("RT_HIP_UPSCALE", std::to_string(upscale).c_str(), 1); // (read by the plug-in: every render() is one rt_hip_render_upscaled frame)
		}
		else if (arg == "--adaptive"sv)
		{
			const char* const threshold = value();
			char* end = nullptr;
			const float parsed = std::strtof(threshold, &end);
			if (end == threshold || *end || !(parsed >= 0.0f) || parsed > 3.0e38f)
			{
				error("--adaptive expects the threshold (a finite number >= 0)");
				return 2;
			}
			adaptive = true;
			::setenv("RT_HIP_ADAPTIVE", threshold, 1); // (read by the plug-in: every render() is one rt_hip_render_adaptive pass)
		}
		else if (arg == "--light"sv)
		{
			lights += (lights.empty() ? "" : ";") + std::string{ value() };
			::setenv("RT_HIP_LIGHTS", lights.c_str(), 1); // (read by the plug-in: the emission table from the scene's material names, RT_HIP_FLAG_EMISSION)
		}
		else if (arg == "--direct-light"sv)
		{
			direct_light = true;
			::setenv("RT_HIP_DIRECT_LIGHT", "1", 1); // (read by the plug-in: RT_HIP_FLAG_DIRECT_LIGHT next to RT_HIP_FLAG_EMISSION)
		}
		else if (arg == "--tonemap"sv)
		{
			tonemap = value();
			rt_hip_tonemap_params parsed{};
			if (rt_hip_tonemap_from_spec(tonemap.c_str(), &parsed) != RT_HIP_OK)
			{
				error("--tonemap expects CURVE[:EXPOSURE], none, reinhard or aces and auto or a positive number (", rt_hip_last_error(), ")");
				return 2;
			}
			::setenv("RT_HIP_TONEMAP", tonemap.c_str(), 1); // (read by the plug-in: every one-shot render() is one rt_hip_render_tonemapped frame)
		}
		else if (arg == "--lens"sv)
		{
			lens = value();
			rt_hip_lens parsed{};
			if (rt_hip_lens_from_spec(lens.c_str(), &parsed) != RT_HIP_OK)
			{
				error("--lens expects aperture=A,focus=F with A >= 0 and F > 0 (", rt_hip_last_error(), ")");
				return 2;
			}
			::setenv("RT_HIP_LENS", lens.c_str(), 1); // (read by the plug-in: rt_hip_set_lens, and RT_HIP_FLAG_THIN_LENS on every one-shot render())
		}
		else if (arg == "--bloom"sv)
		{
			bloom = value();
			rt_hip_bloom_params parsed{};
			if (rt_hip_bloom_from_spec(bloom.c_str(), &parsed) != RT_HIP_OK)
			{
				error("--bloom expects default or KEY=VALUE items separated by ',' with the keys intensity, threshold, knee, scatter and levels (", rt_hip_last_error(), ")");
				return 2;
			}
			::setenv("RT_HIP_BLOOM", bloom.c_str(), 1); // (read by the plug-in: every one-shot render() is one rt_hip_render_bloomed frame)
		}
		else if (arg == "--dolly"sv)
		{
			char trailing = 0;
			if (std::sscanf(value(), "%f,%f,%f%c", &dolly_by[0], &dolly_by[1], &dolly_by[2], &trailing) != 3)
			{
				error("--dolly expects DX,DY,DZ");
				return 2;
			}
			dolly = true;
		}
		else if (arg == "--shared-frame"sv)
			shared_name = value();
		else if (arg == "--rank"sv)
			rank = static_cast<unsigned>(std::strtoul(value(), nullptr, 10));
		else if (arg == "--world"sv)
			world = static_cast<unsigned>(std::strtoul(value(), nullptr, 10));
		else if (arg == "--help"sv || arg == "-h"sv)
		{
			log("usage: rt_headless [--list] [--scene file.toml] [--renderer name] [--size WxH] [--spp N] [--bounces N] [--seed N] [--frames N] [--out file.ppm] [--progressive SAMPLES] [--denoise] [--boxes [--box-bvh]] [--temporal] [--adaptive THRESHOLD] [--upscale FACTOR] [--light KEY=R,G,B]... [--direct-light] [--tonemap CURVE[:EXPOSURE]] [--bloom SPEC] [--lens aperture=A,focus=F] [--dolly DX,DY,DZ] [--shared-frame NAME --rank R --world N]");
			return 0;
		}
		else
		{
			error("unknown argument '", arg, "'");
			return 2;
		}
	}

	log("working directory: ", std::filesystem::current_path().string());
	log("renderers:");
	for (auto& r : renderers::all())
		log("    ", r.name);
	if (list)
		return 0;

	const auto desc = find_renderer_by_name_fuzzy(renderer_name);
	if (!desc)
	{
		error("no known renderer with name '", renderer_name, "'");
		return 1;
	}
	if (upscale)
	{
		const char* const with = progressive ? "--progressive" : (temporal ? "--temporal" : (adaptive ? "--adaptive" : (!lights.empty() ? "--light" : (box_bvh ? "--box-bvh" : nullptr))));
		if (with || std::string_view{ desc->name }.substr(0, 3) != "hip"sv)
		{
			error("--upscale traces one-shot frames of a hip renderer at 1 / FACTOR of the size and rebuilds them (not with --progressive, --temporal, --adaptive, --light or --box-bvh, not '", desc->name, "'): refused with ", with ? with : "this renderer");
			return 2;
		}
	}
	if (!tonemap.empty())
	{
		const char* const with = progressive ? "--progressive" : (temporal ? "--temporal" : (adaptive ? "--adaptive" : (upscale ? "--upscale" : nullptr)));
		const std::string_view name{ desc->name };
		if (with || name.substr(0, 3) != "hip"sv || name == "hip_rasterizer"sv)
		{
			error("--tonemap maps one-shot frames of a hip tracer (not with --progressive, --temporal, --adaptive or --upscale, not '", desc->name, "'): refused with ", with ? with : "this renderer");
			return 2;
		}
	}
	if (!bloom.empty())
	{
		const char* const with = progressive ? "--progressive" : (temporal ? "--temporal" : (adaptive ? "--adaptive" : (upscale ? "--upscale" : nullptr)));
		const std::string_view name{ desc->name };
		if (with || name.substr(0, 3) != "hip"sv || name == "hip_rasterizer"sv)
		{
			error("--bloom blooms one-shot frames of a hip tracer (not with --progressive, --temporal, --adaptive or --upscale, not '", desc->name, "'): refused with ", with ? with : "this renderer");
			return 2;
		}
	}
	if (progressive && (frames_given || std::string_view{ desc->name }.substr(0, 3) != "hip"sv))
	{
		error("--progressive sets the number of frames itself (not with --frames) and needs a hip renderer, not '", desc->name, "'");
		return 2;
	}
	if (adaptive && (frames_given || temporal || boxes || denoise || std::string_view{ desc->name }.substr(0, 3) != "hip"sv))
	{
		error("--adaptive runs the passes of an adaptive accumulation of a hip renderer until it is complete (not with --frames, --temporal, --boxes or --denoise, not '", desc->name, "')");
		return 2;
	}
	if (boxes && (progressive || std::string_view{ desc->name }.substr(0, 3) != "hip"sv))
	{
		error("--boxes traces the scene's boxes in one-shot frames of a hip renderer (not with --progressive, not '", desc->name, "')");
		return 2;
	}
	if (!lights.empty() && (progressive || adaptive || temporal || denoise || boxes || std::string_view{ desc->name }.substr(0, 3) != "hip"sv))
	{
		error("--light makes materials lights in one-shot frames of a hip renderer (not with --progressive, --adaptive, --temporal, --denoise or --boxes, not '", desc->name, "')");
		return 2;
	}
	if (!lens.empty() && (progressive || adaptive || temporal || denoise || upscale || boxes || !lights.empty() || std::string_view{ desc->name }.substr(0, 3) != "hip"sv))
	{
		error("--lens takes one-shot frames of a hip renderer through a thin lens (not with --progressive, --adaptive, --temporal, --denoise, --upscale, --boxes or --light, not '", desc->name, "')");
		return 2;
	}
	if (direct_light && lights.empty())
	{
		error("--direct-light says how the lights of --light are found: lambert surfaces sample the sphere lights directly (not without --light)");
		return 2;
	}
	if (box_bvh && (!boxes || temporal))
	{
		error("--box-bvh says how --boxes reaches the scene's boxes: it needs --boxes, and temporal frames keep the linear scan (not with --temporal)");
		return 2;
	}
	if (temporal && (progressive || std::string_view{ desc->name }.substr(0, 3) != "hip"sv))
	{
		error("--temporal blends whole frames of a hip renderer (not with --progressive, not '", desc->name, "')");
		return 2;
	}
	if (denoise && !progressive && !temporal && !upscale)
	{
		error("--denoise filters the passes of a progressive frame: it needs --progressive SAMPLES (or --temporal)");
		return 2;
	}
	std::unique_ptr<renderer_interface> renderer{ desc->create() };
	log("created renderer: ", desc->name);

	rt::scene scene;
	try
	{
		scene = scene_path.empty() ? rt::scene::load_first_available() : rt::scene::load(scene_path);
	}
	catch (const std::exception& e)
	{
		error(e.what());
		return 1;
	}
	log("scene '", scene.path, "' loaded");
	if (spp)
		scene.samples_per_pixel = spp;
	if (bounces)
		scene.max_bounces = bounces;
	if (progressive)
	{
		const unsigned pass = (progressive + 15u) / 16u * 16u; // (passes are whole chunks of 16 samples: rt_hip_render_progressive rounds up)
		frames = (scene.samples_per_pixel + pass - 1u) / pass;
	}
	else if (adaptive)
		frames = (scene.samples_per_pixel + 15u) / 16u; // (at most: the loop below ends with the accumulation)

	image frame;
	image_view pixels;
	if (shared_name.empty())
	{
		frame = image{ vec2u{ width, height } };
		pixels = image_view{ frame };
	}
	else
	{
		if (!world || rank >= world || shared_name.find('/') != std::string::npos)
		{
			error("--shared-frame NAME needs --rank R --world N with R < N, and a NAME without '/'");
			return 2;
		}
		const size_t bytes = static_cast<size_t>(width) * height * sizeof(uint32_t);
		uint32_t* const shared = map_shared_frame("/" + shared_name + "_frame", rank, bytes);
		if (!shared)
		{
			error("could not map the shared frame '/", shared_name, "_frame'");
			return 1;
		}
		pixels = image_view{ shared, vec2u{ width, height } };
		::setenv("RT_HIP_GROUP", ("/" + shared_name + "_group:" + std::to_string(rank) + ":" + std::to_string(world)).c_str(), 1);
		log("rank ", rank, " of ", world, ": back buffer is the shared mapping /", shared_name, "_frame");
	}
	muu::thread_pool threads;
	double seconds = 0.0;
	for (unsigned f = 0; f < (frames ? frames : 1u); f++)
	{
		if (dolly && f)
			scene.camera.pose(scene.camera.position() + vec3{ dolly_by[0], dolly_by[1], dolly_by[2] }, scene.camera.rotation());
		if (rank == 0)
			pixels.clear(0x000000FFu); // reference src/main.cpp:318 (the other ranks of a shared frame leave it alone)
		const auto t0 = std::chrono::steady_clock::now();
		renderer->render(scene, pixels, threads);
		seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
		if (adaptive)
		{
			// where the accumulation stands: the module's own word on the pass render() has just delivered
			rt_hip_adaptive_info info{};
			if (rt_hip_adaptive_last_info(&info) != RT_HIP_OK)
			{
				error("--adaptive: the renderer did not deliver an adaptive pass (", rt_hip_last_error(), ")");
				return 1;
			}
			const unsigned complete = info.complete, passes = info.passes, count = info.pixels, total = info.samples_total;
			const unsigned long long traced = info.samples_traced;
			if (complete)
			{
				const double budget = static_cast<double>(count) * total;
				std::printf("adaptive: complete after %u passes: samples_traced %llu of pixels x spp = %.0f (%.1f %%)\n", passes, traced, budget, budget > 0.0 ? 100.0 * static_cast<double>(traced) / budget : 0.0);
				std::printf("adaptive: live frame locks %u\n", rt_hip_live_frame_locks()); // (page-locks on this process's frame buffers: none are taken)
				break;
			}
		}
	}
	const double rays = static_cast<double>(width) * height * scene.samples_per_pixel;
	std::printf("%ux%u, %u spp, max_bounces %u: %.3f ms per frame (render() wall clock incl. upload and read-back), %.1f Mrays/s\n",
				width, height, scene.samples_per_pixel, scene.max_bounces, seconds * 1e3, rays / seconds / 1e6);

	if (!shared_name.empty() && rank == 0)
		shm_unlink(("/" + shared_name + "_frame").c_str()); // (every rank has had it mapped since before its first frame)
	if (!out_path.empty() && rank == 0)
	{
		if (!write_ppm(out_path, pixels))
		{
			error("could not write '", out_path, "'");
			return 1;
		}
		log("wrote ", out_path);
	}
	return 0;
}
