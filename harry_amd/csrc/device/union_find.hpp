// The lock-free union-find of the device code (twins.hip: k_cc_*, the components of the encoder's faces; hook.hpp: the shells of a
// render build for shells.hip and the orientation double cover of its patches for orient.hip; shells.hip: the loops of the shells'
// boundaries).  par[i] == i: i is a root; the root of a set is its smallest member, whatever
// order the atomics complete in.  Device-only; every parent word is read and written with agent-scope atomics.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace hry {
namespace dev {

__device__ __forceinline__ uint32_t uf_load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ uint32_t uf_find(uint32_t *par, uint32_t x)
{
	// parents only ever decrease and a face that has got a parent never becomes a root again: a stale read is a valid (higher)
	// ancestor, and the halving store -- a plain one -- can only replace an ancestor by another ancestor
	uint32_t p = uf_load(par + x);
	while (p != x) {
		const uint32_t g = uf_load(par + p);
		if (g != p) __hip_atomic_store(par + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		x = p; p = g;
	}
	return x;
}
__device__ __forceinline__ void uf_unite(uint32_t *par, uint32_t a, uint32_t b)
{
	for (;;) {
		a = uf_find(par, a); b = uf_find(par, b);
		if (a == b) return;
		if (a > b) { const uint32_t t = a; a = b; b = t; }
		const uint32_t old = atomicCAS(par + b, b, a);   // b is a root still: it hangs under the smaller root
		if (old == b) return;
		b = old;
	}
}

// the same in LDS, for the sets a workgroup unites among its own elements before it goes to HBM
__device__ __forceinline__ uint32_t lds_find(uint32_t *par, uint32_t x)
{
	uint32_t p = __hip_atomic_load(par + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
	while (p != x) {
		const uint32_t g = __hip_atomic_load(par + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
		if (g != p) __hip_atomic_store(par + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
		x = p; p = g;
	}
	return x;
}
__device__ __forceinline__ void lds_unite(uint32_t *par, uint32_t a, uint32_t b)
{
	for (;;) {
		a = lds_find(par, a); b = lds_find(par, b);
		if (a == b) return;
		if (a > b) { const uint32_t t = a; a = b; b = t; }
		const uint32_t old = atomicCAS(par + b, b, a);
		if (old == b) return;
		b = old;
	}
}

}   // namespace dev
}   // namespace hry
