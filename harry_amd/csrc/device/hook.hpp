// The two-pass union over a render build's triangles (tri_adjacency.hpp), once for every Graph: shells.hip (ShellGraph, a node a
// triangle) and orient.hip (CoverGraph, the orientation double cover: two).  As k_cc_hook_local / k_cc_hook of twins.hip: triangles
// that lie near each other in the buffer mostly ARE neighbours, so a workgroup first unites its own tile in LDS -- the same lock-free
// union-find (union_find.hpp), no traffic -- and writes every node's local root as its parent; the second pass takes only the
// relations that leave a tile to the union-find in HBM, where a set now arrives as one root per workgroup.  A Graph states
//   kNodes                                 nodes a triangle: node kNodes t + j; with two, j = 1 is the triangle turned
//   side_relation(v, s, other, against)    the relation side s is in charge of: with triangle `other`, along or against
//   next_relation(v, t)                    is triangle t in charge of a relation with t + 1?  (along)
// With one node a relation unites (a, b); with two, along unites (2 a, 2 b) and (2 a + 1, 2 b + 1), against (2 a, 2 b + 1) and
// (2 a + 1, 2 b).  A tile is kHookParents / kNodes triangles: 32 KB of parents in LDS whatever the Graph.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "tri_adjacency.hpp"
#include "union_find.hpp"

namespace hry {
namespace dev {

constexpr uint32_t kHookParents = 8192, kHookThreads = 1024;

// one relation into the parents in LDS (kLds) or in HBM
template <class Graph, bool kLds>
__device__ __forceinline__ void hook_relate(uint32_t *par, uint32_t a, uint32_t b, bool against)
{
	auto unite = [par](uint32_t x, uint32_t y) { if (kLds) lds_unite(par, x, y); else uf_unite(par, x, y); };
	if (Graph::kNodes == 1) { unite(a, b); return; }
	unite(2 * a, 2 * b + (against ? 1u : 0u));
	unite(2 * a + 1, 2 * b + (against ? 0u : 1u));
}

// Every word of par is written here
template <class Graph>
__global__ __launch_bounds__(kHookThreads) void k_hook_local(TriAdjacency v, uint32_t *par)
{
	constexpr uint32_t kTile = kHookParents / Graph::kNodes;
	__shared__ uint32_t l_par[kHookParents];
	const uint32_t base = blockIdx.x * kTile;
	for (uint32_t i = threadIdx.x; i < kHookParents; i += kHookThreads) l_par[i] = i;
	__syncthreads();
	for (uint32_t i = threadIdx.x; i < kTile; i += kHookThreads) {
		const uint32_t t = base + i;
		if (t >= v.ntri) break;
		for (uint32_t k = 0; k < 3; ++k) {
			uint32_t o;
			bool against;
			if (!Graph::side_relation(v, 3 * t + k, o, against)) continue;
			if (o >= v.ntri || o - base >= kTile) continue;   // it leaves the workgroup's triangles: the second pass
			hook_relate<Graph, true>(l_par, i, o - base, against);
		}
		if (i + 1 < kTile && Graph::next_relation(v, t)) hook_relate<Graph, true>(l_par, i, i + 1, false);
	}
	__syncthreads();
	for (uint32_t i = threadIdx.x; i < kHookParents; i += kHookThreads) {   // (the unions are over: a root read is final)
		if (base + i / Graph::kNodes >= v.ntri) break;
		uint32_t x = i, q = l_par[x];
		while (q != x) { x = q; q = l_par[x]; }
		par[Graph::kNodes * (size_t)base + i] = Graph::kNodes * base + x;   // (with two nodes the tile's first is even: a node keeps its low bit)
	}
}

// a lane per side; the first side of a triangle speaks for the triangle's own relation
template <class Graph>
__global__ __launch_bounds__(256) void k_hook(TriAdjacency v, uint32_t *par)
{
	constexpr uint32_t kTile = kHookParents / Graph::kNodes;
	const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
	if (s >= v.n) return;
	const uint32_t t = s / 3, base = t - t % kTile;
	uint32_t o;
	bool against;
	if (Graph::side_relation(v, s, o, against) && o < v.ntri && o - base >= kTile) hook_relate<Graph, false>(par, t, o, against);
	if (s % 3 == 0 && t + 1 - base >= kTile && Graph::next_relation(v, t)) hook_relate<Graph, false>(par, t, t + 1, false);
}

// flag[t] = is the first node of triangle t a root?
template <class Graph>
__global__ __launch_bounds__(256) void k_hook_roots(const uint32_t *par, uint32_t ntri, uint32_t *flag)
{
	const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t < ntri) flag[t] = par[Graph::kNodes * (size_t)t] == Graph::kNodes * t ? 1u : 0u;
}

// the unions, the root flags and their exclusive scan: num[T] = the number of sets, on the device
template <class Graph>
void launch_hook_roots(hipStream_t st, const TriAdjacency &v, uint32_t *par, uint32_t *flag, uint32_t *sums, uint32_t *num)
{
	if (v.ntri) {
		hipLaunchKernelGGL(k_hook_local<Graph>, dim3(blocks_for(v.ntri, kHookParents / Graph::kNodes)), dim3(kHookThreads), 0, st, v, par);
		hipLaunchKernelGGL(k_hook<Graph>, dim3(blocks_for(v.n, 256)), dim3(256), 0, st, v, par);
		hipLaunchKernelGGL(k_hook_roots<Graph>, dim3(blocks_for(v.ntri, 256)), dim3(256), 0, st, (const uint32_t*)par, v.ntri, flag);
	}
	launch_excl_scan(st, flag, v.ntri, sums, num);
}

}   // namespace dev
}   // namespace hry
