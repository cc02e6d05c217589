// Unique edges and adjacency of a render build's triangles (driver: edges.cpp; contract: include/harry_amd.h, hry_edges_build;
// DESIGN.md 7a, "Edges and adjacency").  The items are the 3 T sides of the triangles; dedup.hip's first-occurrence numbering (EdgeKey) has given every side
// its edge (tri_edges), edges numbered by their first side.  Behind it, the pattern of normals.hip: count, scan, scatter, order per
// segment.  Every floating-point operation is an individually rounded IEEE double operation in a fixed order (the tree is built
// with -ffp-contract=off), and there are no floating-point atomics: the bits of every buffer depend on the render build alone.
//   k_edge_count    one counter per edge: its sides (integer atomics)
//   k_scan_*        exclusive scan of the counters into edge_offsets (scan.hip: launch_excl_scan)
//   k_edge_scatter  sides into their edge's segment of edge_sides, in any order (the counters count down as cursors)
//   k_edge_rows     a lane per edge: sorts its segment by side (one or two sides almost everywhere; insertion sort up to kEdgeSegMax),
//                   writes the edge's row, its sides' tri_neighbours and, where asked for, length, cotangent sum and cosine; per
//                   wavefront one integer atomic per class of edge (one side, two, more).  Longer segments are listed for k_edge_hubs
//   k_edge_hubs     a workgroup per listed edge: bitonic sort of the segment where it lies (seg_sort.hpp), tri_neighbours by all threads,
//                   then thread 0 alone does what a lane of k_edge_rows does -- the cotangent sum is the plain left-to-right one at
//                   every length.  The list has a slot for every edge that can qualify (3 T / (kEdgeSegMax + 1)): it cannot overflow
// Streaming work with L2-resident gathers; bytes per triangle of a closed manifold mesh (E = 3 T / 2), after the numbering's 12
// indices + 24 vertex_source gathers per pass: count 12 + 12, scan 18, scatter 12 + 12 + 12 + 12, rows 6 offsets + 24 sides + 12
// edges + 12 tri_neighbours + 24 indices / vertex_source; with geometry 18 out and about 21 position rows of 12 bytes gathered.
#include <hip/hip_runtime.h>

#include "dev_types.hpp"
#include "kernels.hpp"
#include "seg_sort.hpp"

namespace hry {
namespace dev {

namespace {

constexpr uint32_t kEdgeSegMax = 32;

struct D3 { double x, y, z; };

__device__ __forceinline__ D3 position(const EdgesView &v, uint32_t u)
{
	if (u >= v.nout) { const double q = __builtin_nan(""); return D3{ q, q, q }; }   // (no render build writes such an index)
	const float *p = v.pos + (size_t)u * v.pos_stride;
	return D3{ (double)p[0], (double)p[1], (double)p[2] };
}
__device__ __forceinline__ D3 sub(const D3 &a, const D3 &b) { return D3{ a.x - b.x, a.y - b.y, a.z - b.z }; }
__device__ __forceinline__ D3 cross(const D3 &a, const D3 &b) { return D3{ a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x }; }
__device__ __forceinline__ double dot(const D3 &a, const D3 &b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ double length(const D3 &a) { return sqrt(a.x * a.x + a.y * a.y + a.z * a.z); }
__device__ __forceinline__ bool usable(double len) { return len > 0.0 && len < __builtin_inf(); }   // (false for NaN)
__device__ __forceinline__ uint32_t vertex_of(const EdgesView &v, uint32_t u) { return u < v.nout ? v.vsrc[u] : kNoElement; }

// the output vertices side s runs from and to, and its triangle's third corner; false for a side the buffers do not hold
__device__ __forceinline__ bool side_corners(const EdgesView &v, uint32_t s, uint32_t &from, uint32_t &to, uint32_t &other)
{
	if (s >= v.n) return false;
	const uint32_t t = s / 3, k = s - 3 * t;
	from = v.indices[s]; to = v.indices[3 * t + (k + 1) % 3]; other = v.indices[3 * t + (k + 2) % 3];
	return true;
}

// N_t / |N_t| of triangle t; false where it has none
__device__ __forceinline__ bool unit_normal(const EdgesView &v, uint32_t t, D3 &n)
{
	const D3 p0 = position(v, v.indices[3 * t]);
	const D3 N = cross(sub(position(v, v.indices[3 * t + 1]), p0), sub(position(v, v.indices[3 * t + 2]), p0));
	const double len = length(N);
	if (!usable(len)) return false;
	n = D3{ N.x / len, N.y / len, N.z / len };
	return true;
}

// the row of edge e and its geometry from its ordered sides a[0 .. len): one thread
__device__ __forceinline__ void finish_edge(const EdgesView &v, uint32_t e, const uint32_t *a, uint32_t len)
{
	uint32_t from, to, other;
	if (!side_corners(v, a[0], from, to, other)) return;
	const bool swap = vertex_of(v, from) > vertex_of(v, to);
	const uint32_t r0 = swap ? to : from, r1 = swap ? from : to;
	v.edges[(size_t)e * 2] = r0; v.edges[(size_t)e * 2 + 1] = r1;
	if (!v.pos) return;
	v.length[e] = (float)length(sub(position(v, r1), position(v, r0)));
	double S = 0.0;
	for (uint32_t i = 0; i < len; ++i) {
		uint32_t f, t, o;
		double c = 0.0;
		if (side_corners(v, a[i], f, t, o)) {
			const D3 po = position(v, o), u = sub(position(v, f), po), w = sub(position(v, t), po);
			const double l = length(cross(u, w));
			if (usable(l)) c = dot(u, w) / l;
			if (!(fabs(c) < __builtin_inf())) c = 0.0;
		}
		S += c;
	}
	v.cot[e] = (float)(0.5 * S);
	float cs = 2.0f;
	uint32_t f1, t1, o1;
	if (len == 2 && side_corners(v, a[1], f1, t1, o1)) {
		D3 n0, n1;
		if (unit_normal(v, a[0] / 3, n0) && unit_normal(v, a[1] / 3, n1)) {
			const double d = dot(n0, n1);
			const bool against = vertex_of(v, from) == vertex_of(v, f1) && vertex_of(v, to) == vertex_of(v, t1);   // both sides run the same way
			cs = (float)(against ? -d : d);
		}
	}
	v.cos[e] = cs;
}

}   // namespace

__global__ __launch_bounds__(256) void k_edge_count(const uint32_t *tri_edges, uint32_t n, uint32_t ne, uint32_t *count)
{
	const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
	if (s >= n) return;
	const uint32_t e = tri_edges[s];
	if (e < ne) atomicAdd(&count[e], 1u);
}

// (count[e] holds e's sides on entry and counts down: the last free slot of the segment is taken first)
__global__ __launch_bounds__(256) void k_edge_scatter(const uint32_t *tri_edges, uint32_t n, uint32_t ne, const uint32_t *start, uint32_t *count, uint32_t *sides)
{
	const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
	if (s >= n) return;
	const uint32_t e = tri_edges[s];
	if (e >= ne) return;
	const uint32_t k = atomicSub(&count[e], 1u);
	const uint64_t pos = (uint64_t)start[e] + k - 1;
	if (k && pos < n) sides[pos] = s;
}

__global__ __launch_bounds__(256) void k_edge_rows(EdgesView v, uint32_t *hubs, uint32_t hub_cap, uint32_t *classes)
{
	const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
	uint32_t b = 0, len = 0;
	if (e < v.ne) {
		b = v.offsets[e];
		const uint32_t end = v.offsets[e + 1];
		if (end >= b && end <= v.n) len = end - b;
	}
	// the classes, a wavefront at a time (every lane takes part)
	const uint64_t one = __ballot(len == 1), two = __ballot(len == 2), more = __ballot(len > 2);
	if ((threadIdx.x & 63) == 0) {
		if (one) atomicAdd(&classes[0], (uint32_t)__popcll(one));
		if (two) atomicAdd(&classes[1], (uint32_t)__popcll(two));
		if (more) atomicAdd(&classes[2], (uint32_t)__popcll(more));
	}
	if (!len) return;
	if (len > kEdgeSegMax) {
		const uint32_t k = atomicAdd(&hubs[0], 1u);
		if (k < hub_cap) hubs[1 + k] = e;   // (hub_cap: every edge that can have so many sides)
		return;
	}
	uint32_t *a = v.sides + b;
	for (uint32_t i = 1; i < len; ++i) {   // insertion sort by side
		const uint32_t x = a[i];
		uint32_t j = i;
		while (j > 0 && a[j - 1] > x) { a[j] = a[j - 1]; --j; }
		a[j] = x;
	}
	if (len == 2 && a[0] < v.n && a[1] < v.n) { v.neighbours[a[0]] = a[1] / 3; v.neighbours[a[1]] = a[0] / 3; }
	else for (uint32_t i = 0; i < len; ++i) if (a[i] < v.n) v.neighbours[a[i]] = kNoElement;
	finish_edge(v, e, a, len);
}

__global__ __launch_bounds__(256) void k_edge_hubs(EdgesView v, const uint32_t *hubs, uint32_t hub_cap)
{
	const uint32_t listed = min(hubs[0], hub_cap), tid = threadIdx.x;
	for (uint32_t h = blockIdx.x; h < listed; h += gridDim.x) {
		const uint32_t e = hubs[1 + h];
		if (e >= v.ne) continue;
		const uint32_t b = v.offsets[e], end = v.offsets[e + 1];
		if (end < b || end > v.n) continue;
		const uint32_t len = end - b;
		uint32_t *a = v.sides + b;
		block_sort_segment(a, len, tid);
		for (uint32_t i = tid; i < len; i += 256) if (a[i] < v.n) v.neighbours[a[i]] = kNoElement;
		if (tid == 0) finish_edge(v, e, a, len);
		__syncthreads();
	}
}

// ---- launchers
uint32_t edges_hub_capacity(uint32_t nsides) { return nsides / (kEdgeSegMax + 1) + 1; }

void launch_edges(hipStream_t st, const EdgesView &v, uint32_t *count, uint32_t *sums, uint32_t *hubs, uint32_t *classes)
{
	const uint32_t cap = edges_hub_capacity(v.n);
	if (v.n && v.ne) hipLaunchKernelGGL(k_edge_count, dim3(blocks_for(v.n, 256)), dim3(256), 0, st, v.tri_edges, v.n, v.ne, count);
	launch_excl_scan(st, count, v.ne, sums, v.offsets);
	if (!v.n || !v.ne) return;
	hipLaunchKernelGGL(k_edge_scatter, dim3(blocks_for(v.n, 256)), dim3(256), 0, st, v.tri_edges, v.n, v.ne, (const uint32_t*)v.offsets, count, v.sides);
	hipLaunchKernelGGL(k_edge_rows, dim3(blocks_for(v.ne, 256)), dim3(256), 0, st, v, hubs, cap, classes);
	hipLaunchKernelGGL(k_edge_hubs, dim3(std::min<uint32_t>(cap, 1024)), dim3(256), 0, st, v, (const uint32_t*)hubs, cap);
}

}   // namespace dev
}   // namespace hry
