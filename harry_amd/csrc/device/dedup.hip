// First-occurrence numbering on the device: every item gets the id of its key, ids numbered by the key's first item.  Five users:
// the render build's unweld (corners -> output vertices, render.cpp), the ingest's weld (rows -> records, ingest.cpp), the edges
// of a render build (triangle sides -> edges, edges.cpp), the vertices of its shells (corners -> (shell, decoded vertex),
// shells.cpp) and its split vertices (index slots -> (output vertex, smooth group), creases.cpp).  Kernels, wave64, an item per lane:
//   k_dedup_insert<Key>  every item into an open-addressing table of item indices (at least 2 n slots, linear probing)
//   k_dedup_find<Key>    per item the first item of its key; per wavefront of 64 items the mask of first items and their count
//   k_scan_counts        exclusive scan of the wavefront counts by one block (scan.hip: launch_scan_counts)
//   k_dedup_assign       id = dedup_id(first item), and per id its first item (and what `via` holds for it)
//   k_iota               out[i] = i: the numbering where nothing is merged
//
// The protocol.  Keys are never stored: a slot holds an item, and keys are compared by deriving both again from the items (the Key
// policies below).  A slot is claimed by atomicCAS from EMPTY (kNone, the caller's 0xff fill) and from then on belongs to the key of
// the item that claimed it, for good: the only later writes to it are atomicMin by items that compared equal to what it held, so
// every value it ever holds has that key, and the values only decrease.  An item probes from its hash until it has claimed a slot
// or met one of its own key; two items of one key probe the same sequence and, slots never being freed or changing key, cannot
// settle in different slots: the later one meets the earlier one's slot on the way.  So after k_dedup_insert every distinct key owns
// exactly one slot holding its first (smallest) item -- whatever order the atomics completed in.  The table has more slots than
// items, so a probe meets an empty slot within mask + 1 steps.  k_dedup_find runs in a launch of its own, after every insert, and
// reads final values with plain loads.
#include <hip/hip_runtime.h>

#include "dedup_hash.hpp"
#include "dev_types.hpp"
#include "hip_handles.hpp"
#include "kernels.hpp"

namespace hry {
namespace dev {

constexpr uint32_t kNone = 0xffffffffu;

// ---------------------------------------------------------------------------------------------------------
// Key policies: built once per item (view, item), they supply hash() and same(j): has item j this item's key?
// The hashes decide the table's contention and probe lengths: part of the behaviour, bit for bit.  Their arithmetic is in
// dedup_hash.hpp, which host code compiles too.
// ---------------------------------------------------------------------------------------------------------
// unweld: the key of corner c is (org[c], then per corner-target list in list order the record c names, or kNone where the
// region of c's face does not bind the list)
struct UnweldKey {
	using View = UnweldView;
	const UnweldView &u;
	uint32_t c, r;
	static __device__ __forceinline__ uint32_t region_of(const UnweldView &u, uint32_t c)
	{
		const uint32_t f = u.eface[c];
		return f < u.nf ? u.face_reg[f] : kNone;
	}
	static __device__ __forceinline__ uint32_t key_part(const UnweldView &u, uint32_t c, uint32_t r, uint32_t i)
	{
		if (i == 0) return u.org[c];
		const int32_t s = r < u.nregs ? u.cslot[(size_t)r * u.nlists + (i - 1)] : -1;
		return s < 0 ? kNone : u.corner_attr[(size_t)c * u.nb_corner + (uint32_t)s];
	}
	__device__ __forceinline__ UnweldKey(const UnweldView &u, uint32_t c) : u(u), c(c), r(region_of(u, c)) {}
	__device__ __forceinline__ uint32_t hash() const
	{
		uint32_t h = dh::hash_parts_start();
		for (uint32_t i = 0; i <= u.nlists; ++i) h = dh::hash_parts_step(h, key_part(u, c, r, i));   // murmur3's finaliser over the running value
		return h;
	}
	__device__ __forceinline__ bool same(uint32_t e) const
	{
		const uint32_t re = region_of(u, e);
		for (uint32_t i = 0; i <= u.nlists; ++i)
			if (key_part(u, c, r, i) != key_part(u, e, re, i)) return false;
		return true;
	}
};
// weld: the key of row r is its packed record (stride bytes at rec + r * stride)
struct WeldKey {
	using View = WeldView;
	const WeldView &u;
	const uint8_t *a;
	__device__ __forceinline__ WeldKey(const WeldView &u, uint32_t r) : u(u), a(u.rec + (size_t)r * u.stride) {}
	__device__ __forceinline__ uint32_t hash() const
	{
		return dh::hash_bytes(a, u.stride);   // FNV-1a over the bytes, then murmur3's finaliser
	}
	__device__ __forceinline__ bool same(uint32_t e) const
	{
		if (e >= u.n) return false;
		const uint8_t *b = u.rec + (size_t)e * u.stride;
		for (uint32_t k = 0; k < u.stride; ++k)
			if (a[k] != b[k]) return false;
		return true;
	}
};

// edges: the key of side s is the unordered pair of the decoded vertices it joins, lo <= hi (an index outside vsrc stands for itself
// above every vertex: no render build writes one)
struct EdgeKey {
	using View = EdgeView;
	const EdgeView &u;
	uint32_t lo, hi;
	static __device__ __forceinline__ uint32_t vertex_of(const EdgeView &u, uint32_t i) { return i < u.nout ? u.vsrc[i] : kNone; }
	static __device__ __forceinline__ void ends(const EdgeView &u, uint32_t s, uint32_t &lo, uint32_t &hi)
	{
		const uint32_t t = s / 3, k = s - 3 * t;
		const uint32_t a = vertex_of(u, u.indices[s]), b = vertex_of(u, u.indices[3 * t + (k == 2 ? 0 : k + 1)]);
		lo = min(a, b); hi = max(a, b);
	}
	__device__ __forceinline__ EdgeKey(const EdgeView &u, uint32_t s) : u(u) { ends(u, s, lo, hi); }
	__device__ __forceinline__ uint32_t hash() const
	{ return dh::hash_edge(lo, hi); }   // the two ends through murmur3's finaliser, one after the other
	__device__ __forceinline__ bool same(uint32_t e) const
	{
		if (e >= u.n) return false;
		uint32_t l, h;
		ends(u, e, l, h);
		return l == lo && h == hi;
	}
};

// shells: the key of corner c is (the shell of its triangle, the decoded vertex it names)
struct ShellVertexKey {
	using View = ShellVertexView;
	const ShellVertexView &u;
	uint32_t shell, vertex;
	static __device__ __forceinline__ void parts(const ShellVertexView &u, uint32_t c, uint32_t &shell, uint32_t &vertex)
	{
		const uint32_t i = u.indices[c];
		shell = u.tri_shell[c / 3]; vertex = i < u.nout ? u.vsrc[i] : kNone;
	}
	__device__ __forceinline__ ShellVertexKey(const ShellVertexView &u, uint32_t c) : u(u) { parts(u, c, shell, vertex); }
	__device__ __forceinline__ uint32_t hash() const
	{ return dh::hash_shell_vertex(shell, vertex); }   // the vertex, then the shell, through murmur3's finaliser
	__device__ __forceinline__ bool same(uint32_t e) const
	{
		if (e >= u.n) return false;
		uint32_t s, v;
		parts(u, e, s, v);
		return s == shell && v == vertex;
	}
};

// creases: the key of slot s is (the output vertex it names, the root of its smooth group)
struct CreaseKey {
	using View = CreaseSlotView;
	const CreaseSlotView &u;
	uint32_t vertex, root;
	__device__ __forceinline__ CreaseKey(const CreaseSlotView &u, uint32_t s) : u(u), vertex(u.indices[s]), root(u.root[s]) {}
	__device__ __forceinline__ uint32_t hash() const
	{ return dh::hash_crease(vertex, root); }   // the root, then the vertex, through murmur3's finaliser
	__device__ __forceinline__ bool same(uint32_t e) const { return e < u.n && u.indices[e] == vertex && u.root[e] == root; }
};

template <class Key>
__global__ __launch_bounds__(256) void k_dedup_insert(typename Key::View u)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= u.n) return;
	const Key key(u, i);
	uint32_t s = key.hash() & u.mask;
	for (uint32_t probe = 0; probe <= u.mask; ++probe, s = (s + 1) & u.mask) {   // the table has more slots than items: an empty one is met
		uint32_t cur = __hip_atomic_load(&u.table[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		if (cur == kNone) {
			cur = atomicCAS(&u.table[s], kNone, i);
			if (cur == kNone) return;
		}
		if (key.same(cur)) { atomicMin(&u.table[s], i); return; }
	}
}

template <class Key>
__global__ __launch_bounds__(256) void k_dedup_find(typename Key::View u, uint32_t *first_of, uint64_t *masks, uint32_t *counts)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, n = u.n;
	bool first = false;
	if (i < n) {
		const Key key(u, i);
		uint32_t s = key.hash() & u.mask, e = i;
		for (uint32_t probe = 0; probe <= u.mask; ++probe, s = (s + 1) & u.mask) {
			const uint32_t cur = u.table[s];
			if (cur == kNone) break;   // (cannot happen: i itself was inserted)
			if (cur == i || key.same(cur)) { e = cur; break; }
		}
		first_of[i] = e;
		first = e == i;
	}
	const uint64_t b = __ballot(first);
	if ((threadIdx.x & 63) == 0 && (uint64_t)(i >> 6) < ((uint64_t)n + 63) / 64) {
		masks[i >> 6] = b;
		counts[i >> 6] = (uint32_t)__popcll(b);
	}
}

// the id of the key whose first item is e: the first items before e's wavefront, plus those below e inside it
__device__ __forceinline__ uint32_t dedup_id(uint32_t e, const uint64_t *masks, const uint32_t *wave_start)
{
	return wave_start[e >> 6] + (uint32_t)__popcll(masks[e >> 6] & ((1ull << (e & 63)) - 1));
}

// ids[i] = id of item i's key; per id: first_item[id] = the item that defines it, via_out[id] = via[that item] (via may be null)
__global__ __launch_bounds__(256) void k_dedup_assign(uint32_t n, const uint32_t *first_of, const uint64_t *masks, const uint32_t *wave_start, uint32_t nout,
                                                      uint32_t *ids, uint32_t *first_item, const uint32_t *via, uint32_t *via_out)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const uint32_t e = first_of[i];
	if (e >= n) { ids[i] = 0; return; }
	const uint32_t id = dedup_id(e, masks, wave_start);
	ids[i] = id;
	if (e == i && id < nout) {
		first_item[id] = i;
		if (via) via_out[id] = via[i];
	}
}

__global__ __launch_bounds__(256) void k_iota(uint32_t n, uint32_t *out)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) out[i] = i;
}

// ---- launchers
void DedupPlan::reserve(Carve &W, uint32_t items, bool with_ids)
{
	n = items; nw = (uint32_t)(((uint64_t)n + 63) / 64);
	size_t slots = 64;
	while (slots < 2 * (size_t)n) slots <<= 1;
	mask = (uint32_t)(slots - 1);
	at_table = W.reserve(slots * 4); at_first_of = W.reserve((size_t)n * 4); at_masks = W.reserve((size_t)nw * 8);
	at_counts = W.reserve((size_t)nw * 4); at_wave_start = W.reserve(((size_t)nw + 1) * 4);
	own_ids = with_ids;
	if (own_ids) at_ids = W.reserve((size_t)n * 4);
}
void DedupPlan::bind(const Carve &W, void *base)
{
	table = W.ptr<uint32_t>(base, at_table); first_of = W.ptr<uint32_t>(base, at_first_of); masks = W.ptr<uint64_t>(base, at_masks);
	counts = W.ptr<uint32_t>(base, at_counts); wave_start = W.ptr<uint32_t>(base, at_wave_start);
	if (own_ids) ids = W.ptr<uint32_t>(base, at_ids);
}
template <class Key>
static void dedup_count(hipStream_t st, typename Key::View u, const DedupPlan &p)
{
	if (!p.n) return;
	u.n = p.n; u.table = p.table; u.mask = p.mask;   // the kernels' bounds and the grid come from one place
	hipLaunchKernelGGL(k_dedup_insert<Key>, dim3(blocks_for(p.n, 256)), dim3(256), 0, st, u);
	hipLaunchKernelGGL(k_dedup_find<Key>, dim3(blocks_for(p.n, 256)), dim3(256), 0, st, u, p.first_of, p.masks, p.counts);
	launch_scan_counts(st, p.counts, p.nw, p.wave_start);
}
void launch_dedup_count(hipStream_t st, UnweldView u, const DedupPlan &p) { dedup_count<UnweldKey>(st, u, p); }
void launch_dedup_count(hipStream_t st, WeldView u, const DedupPlan &p) { dedup_count<WeldKey>(st, u, p); }
void launch_dedup_count(hipStream_t st, EdgeView u, const DedupPlan &p) { dedup_count<EdgeKey>(st, u, p); }
void launch_dedup_count(hipStream_t st, ShellVertexView u, const DedupPlan &p) { dedup_count<ShellVertexKey>(st, u, p); }
void launch_dedup_count(hipStream_t st, CreaseSlotView u, const DedupPlan &p) { dedup_count<CreaseKey>(st, u, p); }
void launch_dedup_assign(hipStream_t st, const DedupPlan &p, uint32_t nout, uint32_t *first_item, const uint32_t *via, uint32_t *via_out)
{
	if (p.n) hipLaunchKernelGGL(k_dedup_assign, dim3(blocks_for(p.n, 256)), dim3(256), 0, st, p.n, (const uint32_t*)p.first_of, (const uint64_t*)p.masks,
	                            (const uint32_t*)p.wave_start, nout, p.ids, first_item, via, via_out);
}
void launch_iota(hipStream_t st, uint32_t n, uint32_t *out)
{
	if (n) hipLaunchKernelGGL(k_iota, dim3(blocks_for(n, 256)), dim3(256), 0, st, n, out);
}

}   // namespace dev
}   // namespace hry
