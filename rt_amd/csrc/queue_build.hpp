// rt_amd/csrc/queue_build.hpp — what ONE build of render_queue<SCAN, SM, HALF, NP, GC> (kernels.hip) is, said once:
//   * queue_build<SCAN, HALF, NP, GC>: every compile-time property the kernel's body and its helpers (camera_forms.hpp) branch on,
//     with the measurements that led to each build, one paragraph per property, and the combinations that are not built;
//   * queue_words / unpack_words: the values that travel in kernel-argument words a build does not otherwise read (kernels.hpp,
//     rolling_buffers: the contract), as named, typed values — the one place on the device that casts them.
// SM (the scatter table of sm_ray_tracer, RT_HIP_FLAG_SM_MATERIALS, instead of mg_ray_tracer's) changes the shading only and is no
// property of this struct.
#pragma once

#include "kernels.hpp"
#include "box_bvh_scan.hpp"

// waves per SIMD the kernel variants are compiled for (register budget = 512 / waves): measured, see queue_build::waves
#ifndef RT_HIP_WAVES_FEW
#define RT_HIP_WAVES_FEW 7 // scalar-register kernels in general
#endif
// ... and those that hold six or more spheres and seven or more primitives (7 + 0, 8 + 0, 6 + 1, 7 + 1, 6 + 2): 80 registers instead of
// 72 spare them most of their scratch, which costs more than the seventh wave brings — every (spheres, planes) build at 7 and at 6 waves:
// profiles/r05/small_sweep.txt (round 4 had settled the same question build by build: waves_full_ab.txt)
#ifndef RT_HIP_WAVES_MANY
#define RT_HIP_WAVES_MANY 6
#endif
#ifndef RT_HIP_WAVES_RESIDENT
#define RT_HIP_WAVES_RESIDENT 7
#endif
// (RT_HIP_WAVES_DENSE — the streamed kernel of frames that fill the device — and RT_HIP_PERSISTENT_WAVES_CAP: launch_plan.hpp, whose plan reads them too)
// the BVH kernel (scan_bvh, RT_HIP_FLAG_BVH): a pixel tile per wave with a traversal stack of bvh_max_depth words per lane in LDS
// (24 KiB per workgroup)
#ifndef RT_HIP_WAVES_BVH
#define RT_HIP_WAVES_BVH 5
#endif

namespace rt_hip
{
	// waves per SIMD a build is compiled for (the RT_HIP_WAVES_* above)
	// (direct: a direct build of RT_HIP_FLAG_DIRECT_LIGHT, which carries the sample's direct sum, the pending contribution, the aimed sphere and
	// the vertex's normal across the shadow query — about ten more live registers than its light build: a case of its own, one wave fewer)
	// (a lens build of RT_HIP_FLAG_THIN_LENS keeps its scan's count: at 7 and at 5 waves its restart spills nothing, profiles/r33/kernel_registers_lens.txt)
	constexpr int waves_per_simd(int NS, int NP, bool direct = false)
	{
		if (direct)
			return NS == scan_bvh ? RT_HIP_WAVES_BVH - 1 : RT_HIP_WAVES_RESIDENT - 2;
		if (NS == scan_bvh)
			return RT_HIP_WAVES_BVH;
		if (NS == scan_streamed_dense)
			return RT_HIP_WAVES_DENSE;
		if (NS < 0) // scan_tiled, scan_streamed
			return 5;
		if (NS == scan_resident)
			return RT_HIP_WAVES_RESIDENT;
		return NS >= 6 && NS + NP >= 7 ? RT_HIP_WAVES_MANY : RT_HIP_WAVES_FEW;
	}

	template <int SCAN, bool HALF, int NP, bool GC>
	struct queue_build
	{
		// NS: the scan proper, SCAN without what a pass / box / light build's code adds (launch_plan.hpp).  NS > 0: `small` kernel, NS spheres
		// in SGPRs (kernel argument).  NS == scan_resident: `resident` kernel, all primitives in LDS.  NS == scan_tiled: `tiled` kernel — the
		// primitives stream from the SoA columns in HBM/L2 through one LDS tile shared by the workgroup's four waves (coalesced dword per lane
		// per column, radius squared on the way in); every wave still runs its own queue, but the workgroup advances in lock step, one path
		// segment per trip, with barriers around each tile, until all four waves are done.  NS == scan_streamed: `streamed` kernel — the
		// resident loop reading the primitive table from HBM/L2 with wave-uniform scalar loads.  NS == scan_streamed_dense: the same without
		// the cooperative scan of sparse waves, for frames that fill the device (6 waves per SIMD; RT_HIP_WAVES_DENSE, launch_plan.hpp).
		// NS == scan_bvh: the BVH kernel (RT_HIP_FLAG_BVH) — the resident kernel's tile queue, planes scanned from the table in memory,
		// spheres through the hierarchy, one traversal per lane (bvh_scan.hpp; the lanes of a wave hold unrelated rays, and a wave-wide walk
		// would visit the union of their paths).
		static constexpr int NS = scan_of(SCAN);
		static constexpr bool RESIDENT = NS == scan_resident; // all primitives in LDS
		static constexpr bool BVH = NS == scan_bvh;
		// ROLLING ITEMS: the big-scene kernels, launched persistent, whose unit of hand-out is the single item (render_queue's header, handover.hpp)
		static constexpr bool ROLLING = NS < 0 && !BVH;

		// launch bounds: compiled for 7 waves per SIMD.  That raises the compiler's budgets from 64 to 72 vector and from 72
		// to 88 scalar registers.  With 5..8 spheres in SGPRs and in the resident kernel 64 VGPRs mean scratch
		// (dielectric.toml, 7 spheres: 3.85 -> 3.54 ms with 72; resident, 1000 spheres: -2 %).  The 1..4 sphere kernels
		// still fit 64 VGPRs — they keep running 8 waves — and use the extra scalar registers: the lane-mask bookkeeping of
		// the divergent loop no longer spills to VGPR lanes (3.12 -> 3.05 ms).  6 waves are slower everywhere.  The
		// big-scene modes get the registers of 5 waves per SIMD.
		static constexpr int waves = waves_per_simd(NS, NP, scan_has_direct(SCAN));

		// HALF (small and resident kernels, short launches; see choose_queue): the unit of work is HALF a chunk, 8 samples.
		// The chunk sum stays what the contract says — sixteen samples added in sample order — so the lane that traces a
		// chunk's second half cannot add anything up itself: it parks its (up to) eight sample values in the tile's LDS
		// slot, next to the first half's partial sum, and the fold at the end of the wave continues that partial sum with
		// them, in order.  Twice as many, half as long items: what a launch with two or three chunks per lane needs to end
		// evenly (profiles/r03/chunk_probe.txt).
		// chunk-sum slots of a wave's tile (one tile per wave; the rolling kernels keep no sums in LDS): 3 floats per
		// chunk; HALF: 27 — the first half's partial sum, then the second half's eight sample values
		static constexpr uint32_t slot_floats = HALF ? half_chunk_slot_floats : 3u;
		// The kernels that look at a sample's INDEX (half chunks park by it, rolling items publish by it) count indices; the others count
		// windows only (lane_state.hpp).
		static constexpr bool INDEXED = HALF || ROLLING;

		// NP (small kernel only; round 4): the NS scalar-register spheres are FOLLOWED BY NP PLANES (slots NS .. NS + NP - 1 of
		// the kernel argument), so that the reference's own scenes with their ground plane back in (scenes/basic.toml:11-13,
		// scenes/dielectric.toml:17-19) stay on the scalar-operand path.  Which slot is what is known at compile time: no
		// kind check at run time, and the no-plane variants are what they were.  NS + NP <= 8, NP <= 3 (more planes, or planes
		// without a sphere, take the LDS-resident kernel).
		// path segments traced: counted on the scalar unit (one popcount of the tracing lanes per trip) where scalar
		// registers are to spare — the 1..4-sphere kernels; 2 more live SGPRs make the others spill — else per lane
		static constexpr bool SCALAR_SEGMENTS = NS >= 1 && NS + NP <= 4;

		// [NS == scan_resident] from resident_scalar_scan_from spheres on the sphere scan reads the table in memory (scalar loads): only the planes are staged
		// (a build of its own, NP == 1: the scalar-load scan keeps two groups of four spheres in 32 scalar registers, which the
		// LDS-scan build — scenes below the threshold — has for the frame's constants instead)
		static constexpr bool RESIDENT_SCALAR_SCAN = NS == scan_resident && NP == 1;
		// The LDS-resident kernel is built per scan, and its LDS-scan build per camera form too: as ONE kernel it carried the three camera
		// forms' constants AND the scalar-load scan's two groups of four spheres (32 scalar registers), and its loop reloaded the frame's
		// constants from the argument block (30 s_load and 35 v_readlane of spilled scalars per loop body).  NP == 0: the LDS scan (scenes
		// below resident_scalar_scan_from spheres), GC = "the frame is not a pinhole's" (eye or homogeneous form, chosen at run time);
		// NP == 1: the scalar-load scan, all forms at run time as before (split by form it gained nothing and lost 4 % through a tilted
		// camera).  12 spheres 1.23 -> 1.15 ms, 32: 2.06 -> 2.01, basic.toml forced here 2.89 -> 2.72 (profiles/r05/resident_forms_ab.txt).
		static constexpr bool RESIDENT_LDS_SCAN = NS == scan_resident && NP == 0;

		// GC (small kernel only; round 4): the GENERAL camera — an inverse view-projection whose w varies over the frame takes
		// the per-sample division (camera.hpp:42-48) instead of contract v3's affine primary rays.  rt's own matrix is the
		// float inverse of projection x view (camera.hpp:122-137): for a camera that is not axis-aligned its last row comes
		// out with rounding noise in the x and y terms (-4.5e-7 against a w of 0.001 at the far plane: 4.5e-4 relative — not
		// something to round away), i.e. every frame while the user looks around.  Those frames used to fall to the
		// LDS-resident kernel (+35 % on basic.toml); now they keep the scalar-register kernel, in a build of it that carries
		// the 18 scalars of the general form INSTEAD of the 18 of the affine one (both would not fit its scalar registers).
		// The camera form a scalar-register kernel is built for: the pinhole form, or (GC) the eye form.  A matrix without a
		// finite eye (an orthographic frustum: nothing rt's camera can produce) takes the LDS-resident kernel, which carries all
		// three forms — together with seven spheres their scalars do not fit the scalar registers, and hipcc then reloads the
		// SPHERES from the argument block inside the loop (round 5: dielectric.toml through a tilted camera 3.85 ms).
		// (camera_forms.hpp selects the form from these three and the frame's own words.)
		static constexpr bool PINHOLE_ONLY = (NS > 0 || RESIDENT_LDS_SCAN) && !GC, EYE_ONLY = NS > 0 && GC, NEVER_PINHOLE = RESIDENT_LDS_SCAN && GC;

		// PASS (progressive frames; the tile-per-wave whole-chunk kernels only): the launch traces chunks [first_chunk, first_chunk +
		// q.chunks) of every pixel and its fold CONTINUES the pixel's running sum, kept between passes in an accumulator of 3 floats per pixel
		// laid out like out_rgb.  p.samples_per_pixel is the sample count AFTER the pass, so the frame a pass leaves is the one-shot frame at that
		// sample count, bit for bit.  A pass build is named by its scan code — scan_resident_pass, scan_bvh_pass: the kernel's first template
		// argument, of which NS is the scan proper — so that every other instantiation keeps its symbol, and with it its place in the
		// listings the unchanged-kernels check compares (tools/kernel_listing_diff.py).  Neither the accumulator nor first_chunk is an argument
		// of its own: they travel in words these builds do not read (queue_words below; rolling_buffers, kernels.hpp).
		static constexpr bool PASS = scan_is_pass(SCAN);

		// ADAPT (adaptive sampling; scan_resident_adapt, scan_bvh_adapt): a PASS build whose pixels carry a state word — samples
		// held, and "stopped" in bit 31.  Before its first trip the wave ballots its tile's state words into ONE wave-uniform stop mask (a tile
		// holds at most 64 pixels: launch_plan.cpp); an item of a stopped pixel is empty, like an item of a pixel outside the frame, and the
		// fold neither reads nor writes such a pixel; a wave whose in-frame pixels have all stopped leaves at once.  An active pixel folds as
		// PASS does and stores the pass's OWN fold besides (pass_sum: c0, + c1, ... in chunk order — not a difference of running sums).  These
		// builds finish no pixel: adaptive_update (adaptive.hip) does that for the whole frame.  State words and pass sums lie in one block
		// behind the accumulator (rt_hip.h, rt_hip_adaptive_pass_device: accum, state, pass_sum, moments), at offsets frame_params gives: no
		// argument is added.  The first pass (first_chunk == 0) reads no word of the block.
		static constexpr bool ADAPT = scan_is_adaptive(SCAN);

		// BOXES (RT_HIP_FLAG_TRACE_BOXES; the same two kernels, whole chunks only): the query also scans the scene's boxes — staged
		// ONCE per workgroup into LDS behind the scan's own table (the resident kernel's primitives, the hierarchy kernel's stacks), two float4s
		// each, read with wave-uniform addresses after spheres and planes, no votes — and selects among three candidates (scan.hpp).  Named by
		// scan code like the pass builds — scan_resident_boxes, scan_bvh_boxes — so that every other instantiation keeps its symbol and its
		// instructions; the box count and the table's pointer are device_scene's.  (Staged rather than read through scalar loads: the
		// scalar-load build's scalar registers are spoken for by its two groups of four spheres, and 8 KiB of LDS cost no occupancy here.)
		static constexpr bool BOXES = scan_has_boxes(SCAN);

		// BOXTREE (RT_HIP_FLAG_BOX_BVH; the hierarchy kernel only): scan_bvh_boxtree, a box build that stages nothing — the boxes are
		// reached through a hierarchy of their own (box_bvh_scan.hpp), walked per lane on the stack the sphere traversal has finished with; its
		// descriptor lies behind the sphere hierarchy's, where item_sums points, so no argument is added.  A lane the traversal does not take
		// (a zero or non-finite component) scans s.box_bounds in memory; the winning box's corners are read there too.
		static constexpr bool BOXTREE = scan_has_box_tree(SCAN);

		// LIGHTS (RT_HIP_FLAG_EMISSION; the same two kernels, whole chunks only): scan_resident_lights, scan_bvh_lights.  The launch
		// hands these builds a device_scene whose per-primitive shading / scatter pointers are the LIGHT variant of the tables (scene.hip,
		// ensure_light_tables): a hit whose scatter row says scatter_emit ends its sample with throughput * the row's shading.rgb — to the fused
		// tail such a lane is what a lane that ended on the sky is: it draws nothing for the old sample and its stream stands where next_sample
		// puts it.  No argument is added or moved; every other instantiation keeps its symbol and its instructions.
		static constexpr bool LIGHTS = scan_has_lights(SCAN);

		// DIRECT (RT_HIP_FLAG_DIRECT_LIGHT; scan_resident_direct, scan_bvh_direct): a LIGHTS build whose lambert vertices sample the
		// sphere lights.  A lambert lane that would shade takes one trip as an AIMING lane instead: the fused tail's generator step is the vertex
		// rule's (direct_light_rules.hpp), the lane multiplies its throughput by the attenuation at once (the later scatter multiplies by 1),
		// keeps the pending contribution, the aimed sphere and the hit's normal, and its next query is the shadow query from the unchanged origin.
		// After that query it adds the pending contribution if the accepted hit is that very sphere and goes through the tail as an ordinary
		// lambert scatter.  A lane whose rule aims at nothing scatters in the aiming trip itself, with a second step under its own mask.
		// end_sample adds the sample's direct sum in front.  The sampled-light list (at most 256 entries of two float4) is read with per-lane
		// gather loads — each lane picks its own light — from direct_list_bytes in front of the light variant's shading table (kernels.hpp):
		// no argument is added or moved, no LDS is taken; every other instantiation keeps its symbol and its instructions.
		static constexpr bool DIRECT = scan_has_direct(SCAN);

		// LENS (RT_HIP_FLAG_THIN_LENS; scan_resident_lens, scan_bvh_lens; the same two kernels, whole chunks only): a restarting
		// lane takes a SECOND generator step under the restarting lanes' mask — the lens step, directly behind the jitter step; sample 0 draws
		// it from the window's start — maps its two numerators to a point of the unit disk and bends the primary ray it has just made through
		// that point of the lens (lens_rules.hpp).  The ten lens words travel in the frame_params words only the homogeneous camera form reads
		// (mx, my, k_near: lens.hpp, put_lens_words) — a lens frame never takes that form, and these builds do not compile it: no argument is
		// added or moved, every other instantiation keeps its symbol and its instructions.
		static constexpr bool LENS = scan_has_lens(SCAN);

		static_assert(!PASS || !HALF, "passes are built for whole chunks only");
		static_assert(!LENS || (!HALF && scan_of(SCAN) <= 0), "the lens builds are built for whole chunks of the tile-per-wave table kernels only");
		static_assert(!BOXES || !HALF, "the box builds are built for whole chunks only");
		static_assert(!LIGHTS || (!HALF && scan_of(SCAN) <= 0), "the light builds are built for whole chunks of the tile-per-wave table kernels only");
	};

	// The aliased argument words of render_queue (the contract: rolling_buffers, kernels.hpp), unpacked ONCE, behind the kernel's staging
	// barrier.  A value a build has no use for is null / 0.
	struct queue_words
	{
		const device_bvh* bvh;			 // [BVH] the sphere hierarchy's descriptor: travels as item_sums
		const device_box_bvh* box_tree;	 // [BOXTREE] the box hierarchy's, box_bvh_descriptor_offset bytes behind it
		float* accum;					 // [PASS] the pixels' running sums, 3 floats per pixel laid out like out_rgb: travels as pixel_done
		uint32_t first_chunk;			 // [PASS] the chunk of every pixel the pass starts at: travels as q.block_items
	};
	template <class BUILD>
	__device__ __forceinline__ queue_words unpack_words(const queue_params& q, unsigned long long* item_sums, uint32_t* pixel_done)
	{
		queue_words w{};
		if constexpr (BUILD::BVH)
			w.bvh = reinterpret_cast<const device_bvh*>(item_sums);
		if constexpr (BUILD::BOXTREE)
			w.box_tree = reinterpret_cast<const device_box_bvh*>(reinterpret_cast<const unsigned char*>(item_sums) + box_bvh_descriptor_offset);
		if constexpr (BUILD::PASS)
		{
			w.accum = reinterpret_cast<float*>(pixel_done);
			w.first_chunk = q.block_items;
		}
		return w;
	}
	// [ADAPT] the block behind the accumulator (rt_hip.h, rt_hip_adaptive_pass_device: accum, state, pass_sum, moments).  A step of its
	// own, taken where the adaptive builds read their tile's state words: as part of unpack_words it moved their instructions.
	struct adaptive_words
	{
		const uint32_t* pixel_state; // one word per pixel: samples held, "stopped" in bit 31
		float* pass_sums;			 // the pass's own fold, laid out like the accumulator
	};
	__device__ __forceinline__ adaptive_words unpack_adaptive_words(float* accum, const frame_params& p)
	{
		const size_t frame_pixels = static_cast<size_t>(p.width) * p.height;
		return { reinterpret_cast<const uint32_t*>(accum + 3u * frame_pixels), accum + 4u * frame_pixels };
	}
}
