// Consistent winding of a render build's triangles, patch by patch (driver: orient.cpp; contract: include/harry_amd.h,
// hry_orient_build; DESIGN.md 7a, "Orientation").  The adjacency is the edges build's (tri_adjacency.hpp), as in shells.hip.  A
// relation joins two triangles and says whether they agree (along) or one of them has to be turned (against): a joining edge -- exactly two sides, in
// two triangles, between two different decoded vertices -- or two consecutive fan triangles of one face, which are always along.
// The unknown flips are found by a union-find over the orientation double cover: node 2 t is triangle t as wound, node 2 t + 1 the
// same triangle turned.  Along unites (2 a, 2 b) and (2 a + 1, 2 b + 1), against (2 a, 2 b + 1) and (2 a + 1, 2 b).  The root of a set
// is its smallest member (union_find.hpp), so with t0 the lowest triangle of t's patch find(2 t) is 2 t0 or 2 t0 + 1 -- the low bit
// is t's flip relative to t0 -- and the patch cannot be oriented iff 2 t0 + 1 hangs under 2 t0.  No parity travels through a
// concurrent path compression and nothing depends on the order atomics complete in.  wave64, 256 threads a block.
//   k_hook_local / k_hook<CoverGraph>  (hook.hpp) the relations of a side (its joining edge, taken by the edge's second side) and of a
//                              triangle (the next triangle of its face) -- first inside a workgroup's 4096 triangles (8192 nodes) in
//                              LDS, then, for those that leave them, in HBM
//   k_hook_roots + k_scan_*    root flags of the even nodes and their exclusive scan: dense patch numbers in order of the lowest triangle
//   k_or_label                 a lane per triangle: walks 2 t to its root (the unions are over): tri_patch, the relative flip,
//                              patch_first, orientable; triangles, faces and relatively flipped triangles per patch
//   k_or_decide                a lane per patch, HRY_ORIENT_MAJORITY: more than half flipped turns the patch
//   k_or_apply                 a lane per triangle: tri_flip, face_flip, oriented_indices; flipped faces per patch
//   k_or_sides                 a lane per side: open sides and against edges per patch
//   (launch_measures of measures.hip, over the patches and oriented_indices: patch_measures)
//   k_or_outward               a lane per patch, HRY_ORIENT_OUTWARD: a closed orientable patch of negative volume is inverted
//   k_or_turn                  a lane per triangle: the triangles of the inverted patches turned once more
//   k_or_summary               a lane per patch: the five reductions of hry_orient_summary behind P
// Every per-patch count is an integer atomic, aggregated per wavefront first (WaveCounter).  Bytes per triangle: DESIGN.md 7a, "Orientation".
#include <hip/hip_runtime.h>

#include "dev_types.hpp"
#include "hook.hpp"
#include "kernels.hpp"
#include "wave.hpp"
#include "wave_counter.hpp"

namespace hry {
namespace dev {

namespace {

enum : uint32_t { kColTri, kColFace, kColFlipped, kColFlippedFaces, kColAgainst, kColOpen, kColOrientable, kColInverted };

// the two sides s0 < s1 of the edge of side s, where it has exactly two, in two triangles, and s is one of them
__device__ __forceinline__ bool edge_pair(const TriAdjacency &v, uint32_t s, uint32_t &s0, uint32_t &s1)
{
	uint32_t b, end;
	if (!side_segment(v, v.tri_edges[s], b, end) || end < 2 || b != end - 2) return false;   // one side, or more than two
	s0 = v.sides[b]; s1 = v.sides[b + 1];
	return s0 < v.n && s1 < v.n && s0 / 3 != s1 / 3 && (s == s0 || s == s1);
}
// ... do they join?  false: the ends of the edge coincide.  against: both run the same way
__device__ __forceinline__ bool pair_joins(const TriAdjacency &v, uint32_t s0, uint32_t s1, bool &against)
{
	if (vertex_of(v, v.indices[s0]) == vertex_of(v, v.indices[next_corner(s0)])) return false;
	against = same_direction(v, s0, s1);
	return true;
}
// is the edge of side s a joining edge?
__device__ __forceinline__ bool joining_edge(const TriAdjacency &v, uint32_t s, uint32_t &s0, uint32_t &s1, bool &against)
{
	return edge_pair(v, s, s0, s1) && pair_joins(v, s0, s1, against);
}

}   // namespace

// the double cover, two nodes a triangle (hook.hpp)
struct CoverGraph {
	static constexpr uint32_t kNodes = 2;
	// the relation side s is in charge of: the joining edge it is the second side of (a first side stops before the vertices)
	static __device__ __forceinline__ bool side_relation(const TriAdjacency &v, uint32_t s, uint32_t &other, bool &against)
	{
		uint32_t s0, s1;
		if (!edge_pair(v, s, s0, s1) || s != s1 || !pair_joins(v, s0, s1, against)) return false;
		other = s0 / 3;
		return true;
	}
	// ... triangle t is in charge of: the next triangle of its face, along
	static __device__ __forceinline__ bool next_relation(const TriAdjacency &v, uint32_t t) { return t + 1 < v.ntri && v.tri_face[t] == v.tri_face[t + 1]; }
};

// (the unions are over: the walk reads final parents with plain loads and stores nothing into par)
__global__ __launch_bounds__(256) void k_or_label(OrientView v, const uint32_t *par, const uint32_t *num)
{
	const uint32_t col[3] = { kColTri, kColFace, kColFlipped };
	WaveCounter<3> wc;
	for (uint32_t tile = 0; tile < kTiles; ++tile) {
		const uint64_t at = ((uint64_t)blockIdx.x * kTiles + tile) * 256 + threadIdx.x;
		const uint32_t t = (uint32_t)at;
		const bool valid = at < v.ntri;
		uint32_t patch = kNoElement, flip = 0;
		bool new_face = false;
		if (valid) {
			uint32_t x = 2 * t, p = par[x];
			while (p != x && p < 2 * v.ntri) { x = p; p = par[x]; }
			const uint32_t t0 = x >> 1;
			const bool orientable = par[2 * (size_t)t0 + 1] == 2 * t0 + 1;   // the turned lowest triangle is a root of its own
			patch = num[t0];
			flip = orientable ? x & 1u : 0u;
			v.tri_patch[t] = patch;
			v.tri_flip[t] = flip;
			if (t0 == t && patch < v.np) { v.first[patch] = t; v.counts[(size_t)patch * 8 + kColOrientable] = orientable ? 1u : 0u; }
			const uint32_t f = v.tri_face[t];
			new_face = f < v.nf && (t == 0 || v.tri_face[t - 1] != f);   // (the fan triangles of a face are neighbours in the buffer)
		}
		const bool add[3] = { true, new_face, flip != 0 };
		wc.add(v.counts, v.np, valid, patch, add, col);
	}
	wc.flush(v.counts, col);
}

// on a tie the lowest triangle keeps its winding
__global__ __launch_bounds__(256) void k_or_decide(OrientView v, uint32_t *turn)
{
	const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
	if (p >= v.np) return;
	uint32_t *c = v.counts + (size_t)p * 8;
	if (!c[kColOrientable] || 2 * (uint64_t)c[kColFlipped] <= c[kColTri]) return;
	turn[p] = 1;
	c[kColFlipped] = c[kColTri] - c[kColFlipped];
}

__global__ __launch_bounds__(256) void k_or_apply(OrientView v, const uint32_t *turn)
{
	const uint32_t col[1] = { kColFlippedFaces };
	WaveCounter<1> wc;
	for (uint32_t tile = 0; tile < kTiles; ++tile) {
		const uint64_t at = ((uint64_t)blockIdx.x * kTiles + tile) * 256 + threadIdx.x;
		const uint32_t t = (uint32_t)at;
		const bool valid = at < v.ntri;
		uint32_t patch = kNoElement, flip = 0;
		bool new_face = false;
		if (valid) {
			patch = v.tri_patch[t];
			flip = v.tri_flip[t] ^ (patch < v.np ? turn[patch] : 0u);
			v.tri_flip[t] = flip;
			const uint32_t i0 = v.indices[3 * (size_t)t], i1 = v.indices[3 * (size_t)t + 1], i2 = v.indices[3 * (size_t)t + 2];
			v.oriented[3 * (size_t)t] = i0; v.oriented[3 * (size_t)t + 1] = flip ? i2 : i1; v.oriented[3 * (size_t)t + 2] = flip ? i1 : i2;
			const uint32_t f = v.tri_face[t];
			if (f < v.nf) {
				v.face_flip[f] = flip;   // (the fan triangles of a face are related along: they all write the same word)
				new_face = t == 0 || v.tri_face[t - 1] != f;
			}
		}
		const bool add[1] = { new_face && flip != 0 };
		wc.add(v.counts, v.np, valid, patch, add, col);
	}
	wc.flush(v.counts, col);
}

__global__ __launch_bounds__(256) void k_or_sides(OrientView v)
{
	const uint32_t col[2] = { kColAgainst, kColOpen };
	WaveCounter<2> wc;
	for (uint32_t tile = 0; tile < kTiles; ++tile) {
		const uint64_t at = ((uint64_t)blockIdx.x * kTiles + tile) * 256 + threadIdx.x;
		const uint32_t s = (uint32_t)at;
		const bool valid = at < v.n;
		uint32_t s0 = 0, s1 = 0;
		bool against = false;
		const bool joining = valid && joining_edge(v, s, s0, s1, against);
		const bool add[2] = { joining && against && s == s1, valid && !joining };   // (both triangles of a joining edge are one patch)
		wc.add(v.counts, v.np, valid, valid ? v.tri_patch[s / 3] : kNoElement, add, col);
	}
	wc.flush(v.counts, col);
}

// a volume of 0 or NaN leaves the patch; negating the float is exact
__global__ __launch_bounds__(256) void k_or_outward(OrientView v, uint32_t *turn)
{
	const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
	if (p >= v.np) return;
	uint32_t *c = v.counts + (size_t)p * 8;
	float *m = v.measures + (size_t)p * 8;
	const bool inv = c[kColOrientable] && c[kColOpen] == 0 && m[1] < 0.0f;
	turn[p] = inv ? 1u : 0u;
	if (!inv) return;
	c[kColInverted] = 1;
	c[kColFlipped] = c[kColTri] - c[kColFlipped];
	c[kColFlippedFaces] = c[kColFace] - c[kColFlippedFaces];
	m[1] = -m[1];
}

__global__ __launch_bounds__(256) void k_or_turn(OrientView v, const uint32_t *turn)
{
	const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= v.ntri) return;
	const uint32_t patch = v.tri_patch[t];
	if (patch >= v.np || !turn[patch]) return;
	const uint32_t flip = v.tri_flip[t] ^ 1u;
	v.tri_flip[t] = flip;
	const uint32_t a = v.oriented[3 * (size_t)t + 1];
	v.oriented[3 * (size_t)t + 1] = v.oriented[3 * (size_t)t + 2];
	v.oriented[3 * (size_t)t + 2] = a;
	const uint32_t f = v.tri_face[t];
	if (f < v.nf) v.face_flip[f] = flip;
}

// summary: orientable patches, flipped triangles, inverted patches, against edges, against edges in patches that are not orientable
__global__ __launch_bounds__(256) void k_or_summary(const uint32_t *counts, uint32_t np, uint32_t *summary)
{
	const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
	uint32_t c[8] = {};
	if (p < np) for (int k = 0; k < 8; ++k) c[k] = counts[(size_t)p * 8 + k];
	const uint32_t orientable = (uint32_t)__popcll(__ballot(p < np && c[kColOrientable]));
	const uint32_t inverted = (uint32_t)__popcll(__ballot(p < np && c[kColInverted]));
	const uint32_t flipped = wave_sum(c[kColFlipped]), against = wave_sum(c[kColAgainst]);
	const uint32_t remaining = wave_sum(c[kColOrientable] ? 0u : c[kColAgainst]);
	if ((threadIdx.x & 63) == 0) {
		if (orientable) atomicAdd(&summary[0], orientable);
		if (flipped) atomicAdd(&summary[1], flipped);
		if (inverted) atomicAdd(&summary[2], inverted);
		if (against) atomicAdd(&summary[3], against);
		if (remaining) atomicAdd(&summary[4], remaining);
	}
}

// ---- launchers
void launch_orient_roots(hipStream_t st, const OrientView &v, const OrientWork &w) { launch_hook_roots<CoverGraph>(st, v, w.par, w.flag, w.sums, w.num); }

void launch_orient_flips(hipStream_t st, const OrientView &v, const OrientWork &w, bool majority)
{
	if (!v.ntri || !v.np) return;
	const dim3 tiles(blocks_for(v.ntri, 256 * kTiles));
	hipLaunchKernelGGL(k_or_label, tiles, dim3(256), 0, st, v, (const uint32_t*)w.par, (const uint32_t*)w.num);
	if (majority) hipLaunchKernelGGL(k_or_decide, dim3(blocks_for(v.np, 256)), dim3(256), 0, st, v, w.turn);
	hipLaunchKernelGGL(k_or_apply, tiles, dim3(256), 0, st, v, (const uint32_t*)w.turn);
	hipLaunchKernelGGL(k_or_sides, dim3(blocks_for(v.n, 256 * kTiles)), dim3(256), 0, st, v);
}

void launch_orient_outward(hipStream_t st, const OrientView &v, const OrientWork &w)
{
	if (!v.ntri || !v.np || !v.measures) return;
	hipLaunchKernelGGL(k_or_outward, dim3(blocks_for(v.np, 256)), dim3(256), 0, st, v, w.turn);
	hipLaunchKernelGGL(k_or_turn, dim3(blocks_for(v.ntri, 256)), dim3(256), 0, st, v, (const uint32_t*)w.turn);
}

void launch_orient_summary(hipStream_t st, const OrientView &v, const OrientWork &w)
{
	if (v.np) hipLaunchKernelGGL(k_or_summary, dim3(blocks_for(v.np, 256)), dim3(256), 0, st, (const uint32_t*)v.counts, v.np, w.summary);
}

}   // namespace dev
}   // namespace hry
