// rt_amd/csrc/lane_state.hpp — everything a lane of render_queue carries between loop trips (every build; camera_forms.hpp fills its
// ray and base words).
#pragma once

#include "contract.hpp"

namespace rt_hip
{
	// everything a lane carries between loop trips
	struct lane_state
	{
		vec3 origin, dir;	// current ray
		vec3 throughput;	// product of attenuations so far (trace unrolled front to back)
		vec3 chunk_sum;		// running sum of the chunk of samples in flight (:186,193)
		// what a pixel's samples start from (frame_params): pinhole camera — the near-to-far vector through the pixel's
		// corner; eye form — s N' and s N.w of the corner; homogeneous form — (x, y, -, -) of the pixel
		float base_x, base_y, base_z, base_w; // (named words, not an array: hipcc otherwise keeps half of it in scratch)
		stream_keys keys;	// random streams of the pixel (contract.hpp): the key of its hash function and its counter stride
		uint32_t counter;	// random stream position
		// The samples of an item, counted in STREAM POSITIONS: a sample's window starts at stride * (index << 12)
		// (contract.hpp), so "the next sample" is one shift-and-add on the window start and nothing has to be multiplied
		// per restart.  `window` = where the sample in flight started, `window_end` = where the first sample behind the
		// item would start (the stride is odd and an index is below 2^20: distinct samples, distinct windows; index 0 is
		// the one window that starts at position 0).
		uint32_t window, window_end;
		uint32_t sample;	 // [INDEXED kernels only] index of the sample in flight
		uint32_t sample_end; // [INDEXED kernels only] one past the last sample of the item in flight
	};
}
