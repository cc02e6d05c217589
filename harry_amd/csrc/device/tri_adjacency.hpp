// A render build's triangles behind its edges build, as the kernels of shells.hip and orient.hip read them (filled on the host by
// tri_adjacency_of, result_build.cpp), and the helpers over it.  n = 3 T sides: side s = 3 t + k joins indices[s] to
// indices[next_corner(s)]; vsrc[nout]: the decoded vertex of an output vertex; tri_face[T]; tri_edges[n]: the edge of every side;
// offsets[ne + 1] / sides[n]: the CSR of the edges' sides, every segment ascending.  Nothing here is written.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace hry {
namespace dev {

struct TriAdjacency {
	const uint32_t *indices, *vsrc, *tri_face, *tri_edges, *offsets, *sides;
	uint32_t n, ntri, nout, nf, ne;
};

constexpr uint32_t kNoElement = 0xffffffffu;

__device__ __forceinline__ uint32_t vertex_of(const TriAdjacency &v, uint32_t u) { return u < v.nout ? v.vsrc[u] : kNoElement; }
__device__ __forceinline__ uint32_t next_corner(uint32_t s) { return s % 3 == 2 ? s - 2 : s + 1; }

// the segment [b, end) of edge e in sides: false for an edge the buffers do not hold, or a segment that ends outside them.  (It may
// be empty, or begin behind its end: how many sides a caller asks for is the caller's)
__device__ __forceinline__ bool side_segment(const TriAdjacency &v, uint32_t e, uint32_t &b, uint32_t &end)
{
	if (e >= v.ne) return false;
	b = v.offsets[e]; end = v.offsets[e + 1];
	return end <= v.n;
}
// do the sides s0 and s1 run from the same decoded vertex to the same decoded vertex?
__device__ __forceinline__ bool same_direction(const TriAdjacency &v, uint32_t s0, uint32_t s1)
{
	return vertex_of(v, v.indices[s0]) == vertex_of(v, v.indices[s1]) && vertex_of(v, v.indices[next_corner(s0)]) == vertex_of(v, v.indices[next_corner(s1)]);
}

}   // namespace dev
}   // namespace hry
