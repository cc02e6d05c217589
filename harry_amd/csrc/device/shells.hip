// Shells of a render build: the connected pieces of its triangles, their counts and boundary loops (driver: shells.cpp; contract:
// include/harry_amd.h, hry_shells_build; DESIGN.md 7a, "Shells").  The adjacency is the edges build's (tri_adjacency.hpp): every side
// knows its edge (tri_edges) and every edge its sides in ascending order (edge_offsets / edge_sides).  wave64, 256 threads a block.
//   k_hook_local / k_hook<ShellGraph>  (hook.hpp) lock-free union-find over the triangles (union_find.hpp): a side unites its triangle
//                              with the triangle of its edge's first side -- first inside a workgroup's 8192 triangles in LDS, then,
//                              for the sides that leave them, in HBM.  The root of a shell is its lowest triangle
//   k_hook_roots + k_scan_*    root flags and their exclusive scan: dense shell numbers in order of the lowest triangle
//   k_sh_label                 a lane per triangle: walks to its root (the unions are over), tri_shell, face_shell, shell_first;
//                              triangles and faces per shell
//   k_dedup_*<ShellVertexKey>  (dedup.hip) numbers the distinct (shell, decoded vertex) pairs over the 3 T corners
//   k_sh_vertices              a lane per corner: the first corner of a pair counts one vertex for its shell
//   k_loop_min                 a lane per edge: edge_shell, loop_par[e] = e; a boundary edge leaves its number, by integer atomicMin,
//                              in the slot of the pair at either end
//   k_loop_hook                a boundary edge unites with what the slots at its two ends hold: a second union-find, over edges.
//                              A slot belongs to one shell's vertex: loops of two shells that touch at a point stay apart
//   k_sh_edges                 a lane per edge: edges, boundary, nonmanifold, misoriented, loops (a boundary edge that is a root)
//   k_sh_summary               a lane per shell: the five reductions of hry_shells_summary behind S
// Every per-shell count is an integer atomic, aggregated per wavefront first (WaveCounter, wave_counter.hpp): neighbouring triangles, edges and corners
// mostly share a shell, so a wavefront sends one atomic per column.
// The measures of the shells (area, signed volume, box): measures.hip.  Bytes per triangle of a closed manifold mesh: DESIGN.md 7a.
#include <hip/hip_runtime.h>

#include "dev_types.hpp"
#include "hook.hpp"
#include "kernels.hpp"
#include "wave.hpp"
#include "wave_counter.hpp"

namespace hry {
namespace dev {

namespace {

enum : uint32_t { kColTri, kColFace, kColVertex, kColEdge, kColBoundary, kColNonmanifold, kColMisoriented, kColLoops };

// the sides of edge e, any number but none: false for an edge the buffers do not hold
__device__ __forceinline__ bool edge_segment(const TriAdjacency &v, uint32_t e, uint32_t &b, uint32_t &len)
{
	uint32_t end;
	if (!side_segment(v, e, b, end) || end <= b) return false;
	len = end - b;
	return v.sides[b] < v.n;
}

}   // namespace

// a node a triangle: side s hooks its triangle to that of its edge's first side, where that is another (hook.hpp)
struct ShellGraph {
	static constexpr uint32_t kNodes = 1;
	static __device__ __forceinline__ bool side_relation(const TriAdjacency &v, uint32_t s, uint32_t &other, bool &against)
	{
		uint32_t b, len;
		if (!edge_segment(v, v.tri_edges[s], b, len)) return false;
		other = v.sides[b] / 3;
		against = false;
		return other != s / 3;
	}
	static __device__ __forceinline__ bool next_relation(const TriAdjacency&, uint32_t) { return false; }   // (the fan triangles of a face share an edge)
};

// (the unions are over: the walk reads final parents with plain loads and stores nothing into par)
__global__ __launch_bounds__(256) void k_sh_label(ShellsView v, const uint32_t *par, const uint32_t *num)
{
	const uint32_t col[2] = { kColTri, kColFace };
	WaveCounter<2> wc;
	for (uint32_t tile = 0; tile < kTiles; ++tile) {
		const uint64_t at = ((uint64_t)blockIdx.x * kTiles + tile) * 256 + threadIdx.x;
		const uint32_t t = (uint32_t)at;
		const bool valid = at < v.ntri;
		uint32_t shell = kNoElement;
		bool new_face = false;
		if (valid) {
			uint32_t x = t, p = par[x];
			while (p != x && p < v.ntri) { x = p; p = par[x]; }
			shell = num[x];
			v.tri_shell[t] = shell;
			if (x == t && shell < v.ns) v.first[shell] = t;
			const uint32_t f = v.tri_face[t];
			if (f < v.nf) {
				v.face_shell[f] = shell;   // (the fan triangles of a face are one shell: they all write the same word)
				new_face = t == 0 || v.tri_face[t - 1] != f;   // (and they are neighbours in the buffer)
			}
		}
		const bool add[2] = { true, new_face };
		wc.add(v.counts, v.ns, valid, shell, add, col);
	}
	wc.flush(v.counts, col);
}

__global__ __launch_bounds__(256) void k_sh_vertices(ShellsView v, const uint32_t *first_of)
{
	const uint32_t col[1] = { kColVertex };
	WaveCounter<1> wc;
	for (uint32_t tile = 0; tile < kTiles; ++tile) {
		const uint64_t at = ((uint64_t)blockIdx.x * kTiles + tile) * 256 + threadIdx.x;
		const uint32_t c = (uint32_t)at;
		const bool valid = at < v.n;
		const bool add[1] = { valid && first_of[c] == c };
		wc.add(v.counts, v.ns, valid, valid ? v.tri_shell[c / 3] : kNoElement, add, col);
	}
	wc.flush(v.counts, col);
}

__global__ __launch_bounds__(256) void k_loop_min(ShellsView v, const uint32_t *pair_id, uint32_t *slot, uint32_t *loop_par)
{
	const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
	if (e >= v.ne) return;
	loop_par[e] = e;
	uint32_t b, len;
	if (!edge_segment(v, e, b, len)) { v.edge_shell[e] = kNoElement; return; }
	const uint32_t s = v.sides[b];
	v.edge_shell[e] = v.tri_shell[s / 3];
	if (len != 1) return;
	const uint32_t p0 = pair_id[s], p1 = pair_id[next_corner(s)];
	if (p0 < v.n) atomicMin(&slot[p0], e);
	if (p1 < v.n) atomicMin(&slot[p1], e);
}

__global__ __launch_bounds__(256) void k_loop_hook(ShellsView v, const uint32_t *pair_id, const uint32_t *slot, uint32_t *loop_par)
{
	const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
	uint32_t b, len;
	if (!edge_segment(v, e, b, len) || len != 1) return;
	const uint32_t s = v.sides[b];
	const uint32_t p0 = pair_id[s], p1 = pair_id[next_corner(s)];
	const uint32_t a0 = p0 < v.n ? slot[p0] : kNoElement, a1 = p1 < v.n ? slot[p1] : kNoElement;
	if (a0 < v.ne && a0 != e) uf_unite(loop_par, e, a0);
	if (a1 < v.ne && a1 != e) uf_unite(loop_par, e, a1);
}

__global__ __launch_bounds__(256) void k_sh_edges(ShellsView v, const uint32_t *loop_par)
{
	const uint32_t col[5] = { kColEdge, kColBoundary, kColNonmanifold, kColMisoriented, kColLoops };
	WaveCounter<5> wc;
	for (uint32_t tile = 0; tile < kTiles; ++tile) {
		const uint64_t at = ((uint64_t)blockIdx.x * kTiles + tile) * 256 + threadIdx.x;
		const uint32_t e = at < v.ne ? (uint32_t)at : kNoElement;
		uint32_t b = 0, len = 0, shell = kNoElement;
		bool valid = edge_segment(v, e, b, len), against = false, root = false;
		if (valid) {
			shell = v.edge_shell[e];
			if (len == 1) root = loop_par[e] == e;
			if (len == 2 && v.sides[b + 1] < v.n) {   // both sides run from the same decoded vertex to the same decoded vertex
				const uint32_t s0 = v.sides[b], s1 = v.sides[b + 1];
				against = vertex_of(v, v.indices[s0]) == vertex_of(v, v.indices[s1]) &&
				          vertex_of(v, v.indices[next_corner(s0)]) == vertex_of(v, v.indices[next_corner(s1)]);
			}
		}
		const bool add[5] = { true, len == 1, len > 2, against, root };
		wc.add(v.counts, v.ns, valid, shell, add, col);
	}
	wc.flush(v.counts, col);
}

// summary: closed, nonmanifold, misoriented (shells), loops (sum), largest (triangles)
__global__ __launch_bounds__(256) void k_sh_summary(const uint32_t *counts, uint32_t ns, uint32_t *summary)
{
	const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
	uint32_t c[8] = {};
	if (s < ns) for (int k = 0; k < 8; ++k) c[k] = counts[(size_t)s * 8 + k];
	const bool valid = s < ns;
	const uint32_t closed = (uint32_t)__popcll(__ballot(valid && c[kColBoundary] == 0 && c[kColNonmanifold] == 0));
	const uint32_t nonman = (uint32_t)__popcll(__ballot(valid && c[kColNonmanifold] > 0));
	const uint32_t mis = (uint32_t)__popcll(__ballot(valid && c[kColMisoriented] > 0));
	const uint32_t loops = wave_sum(c[kColLoops]), largest = wave_max(c[kColTri]);
	if ((threadIdx.x & 63) == 0) {
		if (closed) atomicAdd(&summary[0], closed);
		if (nonman) atomicAdd(&summary[1], nonman);
		if (mis) atomicAdd(&summary[2], mis);
		if (loops) atomicAdd(&summary[3], loops);
		if (largest) atomicMax(&summary[4], largest);
	}
}

// ---- launchers
void launch_shells_roots(hipStream_t st, const ShellsView &v, const ShellsWork &w) { launch_hook_roots<ShellGraph>(st, v, w.par, w.flag, w.sums, w.num); }

void launch_shells_label(hipStream_t st, const ShellsView &v, const ShellsWork &w)
{
	if (v.ntri) hipLaunchKernelGGL(k_sh_label, dim3(blocks_for(v.ntri, 256 * kTiles)), dim3(256), 0, st, v, (const uint32_t*)w.par, (const uint32_t*)w.num);
}

void launch_shells_counts(hipStream_t st, const ShellsView &v, const ShellsWork &w)
{
	if (!v.ntri || !v.ns) return;
	hipLaunchKernelGGL(k_sh_vertices, dim3(blocks_for(v.n, 256 * kTiles)), dim3(256), 0, st, v, w.pair_first_of);
	if (v.ne) {
		const dim3 grid(blocks_for(v.ne, 256));
		hipLaunchKernelGGL(k_loop_min, grid, dim3(256), 0, st, v, (const uint32_t*)w.pair_id, w.slot, w.loop_par);
		hipLaunchKernelGGL(k_loop_hook, grid, dim3(256), 0, st, v, (const uint32_t*)w.pair_id, (const uint32_t*)w.slot, w.loop_par);
		hipLaunchKernelGGL(k_sh_edges, dim3(blocks_for(v.ne, 256 * kTiles)), dim3(256), 0, st, v, (const uint32_t*)w.loop_par);
	}
	hipLaunchKernelGGL(k_sh_summary, dim3(blocks_for(v.ns, 256)), dim3(256), 0, st, (const uint32_t*)v.counts, v.ns, w.summary);
}

}   // namespace dev
}   // namespace hry
