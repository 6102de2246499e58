// rt_amd/csrc/handover.hpp — how the rolling kernels (scan_tiled, scan_streamed, scan_streamed_dense: items drawn from ONE launch-wide
// sequence, a pixel's chunks traced by different waves) draw their items and hand chunk sums from wave to wave through HBM:
// fetch_items, publish_sum / read_sum / read_sums8, count_arrival / last_arrival.  The tile-per-wave builds use none of it.
// The accesses are written out in gfx950 assembly; the argument for their ordering is made below, once.
#pragma once

#include "contract.hpp"
#include "kernels.hpp"

namespace rt_hip
{
	__device__ __forceinline__ unsigned long long fetch_items(device_counters* counters, uint32_t count) // call converged
	{
		unsigned long long base = 0;
		if ((threadIdx.x & 63u) == 0)
			base = atomicAdd(&counters->next_item, static_cast<unsigned long long>(count));
		const uint32_t lo = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(base));
		const uint32_t hi = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(base >> 32));
		return (static_cast<unsigned long long>(hi) << 32) | lo;
	}

	// A value (a chunk's sum, or one sample's) on its way between waves: 16 bytes per slot, ONE store and ONE load, both
	// past this CU's L1 and this XCD's L2 (... sc1: the XCDs' L2s are not coherent with one another).
	//   Round 3 wrote a slot as an 8-byte and a 4-byte agent-scope atomic store and read it back the same way: two memory
	//   requests each way per sample, tallied by the counters at 32 bytes apiece (config 5: WRITE_SIZE 8.9 GB for 2.1 GB of
	//   payload).  hipcc has no 16-byte atomic, so the single dwordx4 access is written out
	//   (the A/B against the old form: profiles/r04/ab_publish_16_bytes.txt).
	// THE HAND-OVER PROTOCOL (publish -> count the arrival -> the last arrival reads), as the hardware executes it:
	//   1. the producer's stores are write-through (sc1): when `s_waitcnt vmcnt(0)` lets the wave go on, they have been
	//      acknowledged by the memory side (gfx950 counts stores in vmcnt and acknowledges a write-through store when it
	//      has left the L2 for the fabric);
	//   2. the arrival is an agent-scope atomic add, executed at the memory side, issued after (1) in program order;
	//   3. the consumer's loads are issued after the atomic's RETURN VALUE has come back (they depend on the branch on
	//      it) and bypass the non-coherent caches (sc1): they observe memory as of a moment after every producer's (1).
	// That is an argument from the gfx950 ISA, not from the HIP memory model: in the model's terms the
	// arrival would be a release (buffer_wbl2 sc1 + s_waitcnt in front of the atomic) and the last arrival an acquire
	// (buffer_inv sc1 behind it).  RT_HIP_MODEL_ORDERING=1 builds exactly that; measured, it costs the streamed kernel
	// its scene — buffer_inv sc1 drops the XCD's L2 copy of the sphere table once per finished pixel
	// (profiles/r04/arrival_ordering_ab.txt) — so the ISA-level form stays, and this file refuses to be compiled for
	// anything but gfx950, where the argument was made and the suite's parity tests exercise it.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "handover.hpp: the cross-wave hand-over of the rolling kernels relies on gfx950's store acknowledgement and sc1 semantics"
#endif
	typedef float v4f __attribute__((ext_vector_type(4)));

	__device__ __forceinline__ void publish_sum(unsigned long long* slot, vec3 sum)
	{
		const v4f value = { sum.x, sum.y, sum.z, 0.0f };
		// The two wait states behind the store are part of it: a VMEM store of more than 64 bits reads its data registers
		// after issue, and a vector instruction that overwrites them within two wait states corrupts the stored value
		// (gfx940+ "VMEM store data hazard").  The compiler pads its own stores; it cannot see into this one — found the
		// hard way: the sm kernels' next instruction recycled the value's upper half for an address, and z arrived as a
		// pointer's low word (profiles/r04/case0_bisect.txt).
		asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" : : "v"(slot), "v"(value) : "memory");
	}
	__device__ __forceinline__ vec3 read_sum(unsigned long long* slot)
	{
		v4f value;
		asm volatile("global_load_dwordx4 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=v"(value) : "v"(slot) : "memory");
		return { value.x, value.y, value.z };
	}
	// eight consecutive slots, the loads in flight together
	__device__ __forceinline__ void read_sums8(unsigned long long* first, vec3 (&out)[8])
	{
		v4f v0, v1, v2, v3, v4, v5, v6, v7;
		asm volatile("global_load_dwordx4 %0, %8, off sc1\n\t"
					 "global_load_dwordx4 %1, %8, off offset:16 sc1\n\t"
					 "global_load_dwordx4 %2, %8, off offset:32 sc1\n\t"
					 "global_load_dwordx4 %3, %8, off offset:48 sc1\n\t"
					 "global_load_dwordx4 %4, %8, off offset:64 sc1\n\t"
					 "global_load_dwordx4 %5, %8, off offset:80 sc1\n\t"
					 "global_load_dwordx4 %6, %8, off offset:96 sc1\n\t"
					 "global_load_dwordx4 %7, %8, off offset:112 sc1\n\t"
					 "s_waitcnt vmcnt(0)"
					 : "=&v"(v0), "=&v"(v1), "=&v"(v2), "=&v"(v3), "=&v"(v4), "=&v"(v5), "=&v"(v6), "=&v"(v7)
					 : "v"(first)
					 : "memory");
		out[0] = { v0.x, v0.y, v0.z }, out[1] = { v1.x, v1.y, v1.z }, out[2] = { v2.x, v2.y, v2.z }, out[3] = { v3.x, v3.y, v3.z };
		out[4] = { v4.x, v4.y, v4.z }, out[5] = { v5.x, v5.y, v5.z }, out[6] = { v6.x, v6.y, v6.z }, out[7] = { v7.x, v7.y, v7.z };
	}

	// the arrival of an item at its pixel's counter, and what the lane that brings the LAST item does before it reads
	__device__ __forceinline__ uint32_t count_arrival(uint32_t* counter)
	{
#ifdef RT_HIP_MODEL_ORDERING
		return __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
#else
		asm volatile("s_waitcnt vmcnt(0) ; what was published has left before the arrival is counted" ::: "memory");
		return __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
	}
	__device__ __forceinline__ void last_arrival()
	{
#ifdef RT_HIP_MODEL_ORDERING
		__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
#else
		__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); // (no instruction: keeps the loads below the counter's answer)
#endif
	}
}
