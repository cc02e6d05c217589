// The hash arithmetic of the first-occurrence numbering's key policies (dedup.hip), usable from HIP kernels and from plain host
// code: tests/native/dedup_hash_check.cpp prints these functions' values, and tests/dedup_ref.py restates them in numpy.
// The hashes decide the table's contention and probe lengths: part of the behaviour, bit for bit.
#pragma once
#include <cstdint>

#ifndef HRY_HD
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define HRY_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define HRY_HD inline
#endif
#endif

namespace hry {
namespace dh {

// murmur3's finaliser
HRY_HD uint32_t fmix(uint32_t h)
{
	h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
	return h;
}

// one more key part into a running value, then the finaliser
HRY_HD uint32_t mix_part(uint32_t h, uint32_t part)
{
	h ^= part + 0x7f4a7c15u + (h << 6) + (h >> 2);
	return fmix(h);
}

// a record of `stride` bytes (WeldKey): FNV-1a over the bytes, then the finaliser
HRY_HD uint32_t hash_bytes(const uint8_t *a, uint32_t stride)
{
	uint32_t h = 0x811c9dc5u;
	for (uint32_t k = 0; k < stride; ++k) h = (h ^ a[k]) * 0x01000193u;
	return fmix(h);
}

// two parts through the finaliser, one after the other
HRY_HD uint32_t hash_pair(uint32_t first, uint32_t second)
{
	return mix_part(fmix(first * 0x9e3779b1u), second);
}
// ... in each policy's own order: EdgeKey the two ends, lo <= hi; ShellVertexKey the vertex, then the shell; CreaseKey the root,
// then the vertex
HRY_HD uint32_t hash_edge(uint32_t lo, uint32_t hi) { return hash_pair(lo, hi); }
HRY_HD uint32_t hash_shell_vertex(uint32_t shell, uint32_t vertex) { return hash_pair(vertex, shell); }
HRY_HD uint32_t hash_crease(uint32_t vertex, uint32_t root) { return hash_pair(root, vertex); }

// the running value over a list of parts (UnweldKey: org, then one part per corner-target list): start, then step per part
HRY_HD uint32_t hash_parts_start() { return 0x9e3779b9u; }
HRY_HD uint32_t hash_parts_step(uint32_t h, uint32_t part) { return mix_part(h, part); }

}   // namespace dh
}   // namespace hry
