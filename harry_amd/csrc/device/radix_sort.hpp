// A device-wide stable radix sort of (32-bit key, 32-bit value) pairs, least significant digit first, 8 bits a pass (users: bvh.hip;
// seg_sort.hpp orders one segment inside one workgroup, this orders any number of items across the grid).  One pass is
//   k_radix_count    a workgroup per tile of kRadixTile items: how many of them carry each of the 256 digits (integer atomics in LDS:
//                    sums of ones, whatever the order), written digit-major -- counts[digit * tiles + tile]
//   k_scan_*         the exclusive scan of those 256 * tiles counters (scan.hip: launch_excl_scan): where the items of (digit, tile)
//                    begin in the output
//   k_radix_scatter  the same tile again: an item's place is that start plus its rank among the tile's items of its digit, in item
//                    order.  The rank comes from ballots: eight of them give the lanes of the wavefront with the same digit, a
//                    popcount below the lane the rank inside the wavefront, the popcount of the whole mask the wavefront's count, and
//                    one thread per digit adds the sixteen (round, wavefront) counts up in order.  No atomic decides a place, so a
//                    pass is stable and the output depends on the keys alone.
// The number of items is read from device memory (n_dev): a caller that compacts on the device sorts what it kept without a trip to
// the host; cap bounds it on the host and sizes the grid.  Device-only; launchers at the end.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.hpp"

namespace hry {
namespace dev {

constexpr uint32_t kRadixBlock = 256, kRadixRounds = 4, kRadixTile = kRadixBlock * kRadixRounds, kRadixDigits = 256;

inline uint32_t radix_tiles(uint32_t cap) { return blocks_for(cap, kRadixTile); }
// the words of scratch a pass needs for a sort of at most cap items: the counters, their scan (one more word: the total) and the
// scan's sums
inline size_t radix_count_words(uint32_t cap) { return (size_t)kRadixDigits * radix_tiles(cap); }
inline size_t radix_scratch_words(uint32_t cap) { return 2 * radix_count_words(cap) + 1 + scan_sums_words((uint32_t)radix_count_words(cap)); }

static __global__ __launch_bounds__(kRadixBlock) void k_radix_count(const uint32_t *key, const uint32_t *n_dev, uint32_t shift, uint32_t tiles, uint32_t *counts)
{
	__shared__ uint32_t s_hist[kRadixDigits];
	const uint32_t n = *n_dev, base = blockIdx.x * kRadixTile;
	s_hist[threadIdx.x] = 0;
	__syncthreads();
#pragma unroll
	for (uint32_t r = 0; r < kRadixRounds; ++r) {
		const uint32_t i = base + r * kRadixBlock + threadIdx.x;
		if (i < n) atomicAdd(&s_hist[(key[i] >> shift) & 255u], 1u);
	}
	__syncthreads();
	counts[(size_t)threadIdx.x * tiles + blockIdx.x] = s_hist[threadIdx.x];
}

static __global__ __launch_bounds__(kRadixBlock) void k_radix_scatter(const uint32_t *key, const uint32_t *val, const uint32_t *n_dev, uint32_t shift, uint32_t tiles,
                                                                const uint32_t *starts, uint32_t *key_out, uint32_t *val_out)
{
	constexpr uint32_t kSlots = kRadixRounds * (kRadixBlock / 64);   // (round, wavefront) in item order
	__shared__ uint32_t s_cnt[kSlots][kRadixDigits];
	const uint32_t n = *n_dev, base = blockIdx.x * kRadixTile, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	for (uint32_t s = 0; s < kSlots; ++s) s_cnt[s][threadIdx.x] = 0;
	__syncthreads();
	uint32_t k[kRadixRounds], rank[kRadixRounds];   // (indexed by unrolled loops only: registers)
#pragma unroll
	for (uint32_t r = 0; r < kRadixRounds; ++r) {
		const uint32_t i = base + r * kRadixBlock + threadIdx.x;
		const bool have = i < n;
		k[r] = have ? key[i] : 0u;
		const uint32_t d = (k[r] >> shift) & 255u;
		unsigned long long same = __ballot(have);
#pragma unroll
		for (uint32_t b = 0; b < 8; ++b) {
			const unsigned long long set = __ballot((d >> b) & 1u);
			same &= (d >> b) & 1u ? set : ~set;
		}
		rank[r] = (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
		if (have && rank[r] == 0) s_cnt[r * (kRadixBlock / 64) + wave][d] = (uint32_t)__popcll(same);
	}
	__syncthreads();
	{
		uint32_t run = starts[(size_t)threadIdx.x * tiles + blockIdx.x];
		for (uint32_t s = 0; s < kSlots; ++s) { const uint32_t c = s_cnt[s][threadIdx.x]; s_cnt[s][threadIdx.x] = run; run += c; }
	}
	__syncthreads();
#pragma unroll
	for (uint32_t r = 0; r < kRadixRounds; ++r) {
		const uint32_t i = base + r * kRadixBlock + threadIdx.x;
		if (i >= n) continue;
		const uint32_t at = s_cnt[r * (kRadixBlock / 64) + wave][(k[r] >> shift) & 255u] + rank[r];
		if (at < n) { key_out[at] = k[r]; val_out[at] = val[i]; }   // (at < n always: the counters sum to n)
	}
}

// sorts the first *n_dev (at most cap) pairs of (key_a, val_a) by the key's bits [0, 8 * passes), stably.  key_b / val_b: as large;
// scratch: radix_scratch_words(cap) words.  An even number of passes leaves the result in (key_a, val_a), an odd one in (key_b, val_b)
inline void launch_radix_sort(hipStream_t st, uint32_t *key_a, uint32_t *val_a, uint32_t *key_b, uint32_t *val_b, const uint32_t *n_dev, uint32_t cap, int passes,
                              uint32_t *scratch)
{
	if (!cap) return;
	const uint32_t tiles = radix_tiles(cap), words = (uint32_t)radix_count_words(cap);
	uint32_t *counts = scratch, *starts = counts + words, *sums = starts + words + 1;
	for (int p = 0; p < passes; ++p) {
		hipLaunchKernelGGL(k_radix_count, dim3(tiles), dim3(kRadixBlock), 0, st, (const uint32_t*)key_a, n_dev, (uint32_t)(8 * p), tiles, counts);
		launch_excl_scan(st, counts, words, sums, starts);
		hipLaunchKernelGGL(k_radix_scatter, dim3(tiles), dim3(kRadixBlock), 0, st, (const uint32_t*)key_a, (const uint32_t*)val_a, n_dev, (uint32_t)(8 * p), tiles,
		                   (const uint32_t*)starts, key_b, val_b);
		std::swap(key_a, key_b); std::swap(val_a, val_b);
	}
}

}   // namespace dev
}   // namespace hry
