// The wavefront-aggregated counter of the per-label counts (shells.hip: shell_counts; orient.hip: patch_counts; the labels' measures
// are measures.hip's, the adjacency both read tri_adjacency.hpp).  Device-only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace hry {
namespace dev {

// counts[label][col[i]] += the lanes with valid && add[i], for every label the wavefront holds; a row of counts has 8 columns.  The
// sums of the label met last stay in registers (everything here is uniform over the wavefront) over the kTiles tiles of 256 items a
// block takes one after the other, and go out as one atomic per column when another label is met and at the end: with one shell of a
// million triangles every wavefront would otherwise queue at the same eight words.  Every lane of the wavefront calls add() and flush()
constexpr uint32_t kTiles = 8;
template <int N>
struct WaveCounter {
	static constexpr uint32_t kNone = 0xffffffffu;
	uint32_t shell = kNone, acc[N] = {};
	__device__ __forceinline__ void flush(uint32_t *counts, const uint32_t (&col)[N])
	{
		if (shell == kNone || (threadIdx.x & 63) != 0) return;
#pragma unroll
		for (int i = 0; i < N; ++i) if (acc[i]) atomicAdd(&counts[(size_t)shell * 8 + col[i]], acc[i]);
	}
	__device__ __forceinline__ void add(uint32_t *counts, uint32_t ns, bool valid, uint32_t sh, const bool (&add)[N], const uint32_t (&col)[N])
	{
		valid = valid && sh < ns;
		unsigned long long todo = __ballot(valid);
		while (todo) {
			const int leader = __ffsll((long long)todo) - 1;
			const uint32_t s0 = (uint32_t)__shfl((int)sh, leader, 64);
			const bool mine = valid && sh == s0;
			if (s0 != shell) {
				flush(counts, col);
				shell = s0;
#pragma unroll
				for (int i = 0; i < N; ++i) acc[i] = 0;
			}
#pragma unroll
			for (int i = 0; i < N; ++i) acc[i] += (uint32_t)__popcll(__ballot(mine && add[i]));
			todo &= ~__ballot(mine);
		}
	}
};

}   // namespace dev
}   // namespace hry
