// Meshes from device buffers (driver: ingest.cpp; contract: include/harry_amd.h, hry_mesh_from_device).  Streaming kernels, wave64,
// one element per lane and consecutive lanes on consecutive output words (coalesced stores):
//   k_ingest_degrees   a lane per face: degree check, the set of degrees, per wavefront the sum of its 64 degrees, a 64-bit total
//   k_ingest_foff      a lane per face: face_off[f + 1] = scanned wave sum + the prefix of the degrees inside the wavefront
//   k_ingest_foff_tri  every face a triangle: face_off[f] = 3f
//   k_ingest_org       a lane per half-edge: the index, range-checked, through the weld map when welding
//   k_ingest_pack      a lane per 4-byte word of a list's AoS records: strided columns gathered into the list's layout
// and for meshes with corner lists (hry_mesh_from_device_corners):
//   k_ingest_corner_attr  a lane per word of corner_attr: the corner's row in the slot's list, range-checked, through that list's weld map
//   k_region_first / k_region_rank / k_ingest_face_region   a material per face -> regions numbered by first occurrence
// The weld (one output record per distinct packed record, in first-occurrence order over the input rows) is dedup.hip's numbering
// over a WeldView's keys, vtx_attr[v] = v its k_iota; the one-block scan of the wave sums is scan.hip's launch_scan_counts, the sums
// and prefixes inside a wavefront wave.hpp's.
// The checks of the input raise bits of one status word (vector atomics, once per wavefront); the host reads it back once.  Offsets
// computed from bad degrees are stored but never used for an address: the host refuses the mesh first.
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "wave.hpp"

namespace hry {
namespace dev {

constexpr uint32_t kNone = 0xffffffffu;

// ---------------------------------------------------------------------------------------------------------
// face offsets from uint8 degrees: per wavefront of 64 faces the sum of its degrees (at most 64 x 255, a u32), scanned by
// launch_scan_counts (scan.hip), then the prefix inside the wavefront.  The 64-bit total is summed separately (per block in LDS, then one atomic
// per block): the host compares it with n_indices before it trusts any u32 offset, so degrees whose sum passes 2^32 cannot wrap.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_ingest_degrees(const uint8_t *deg, uint32_t nf, uint32_t *wave_sums, IngestStatus *st)
{
	__shared__ uint32_t mask[8];
	__shared__ unsigned long long bsum;
	if (threadIdx.x < 8) mask[threadIdx.x] = 0;
	if (threadIdx.x == 0) bsum = 0;
	__syncthreads();
	const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t d = f < nf ? deg[f] : 0;
	if (f < nf) atomicOr(&mask[d >> 5], 1u << (d & 31));
	const uint64_t bad = __ballot(f < nf && d < 3);
	const uint32_t s = wave_sum(d);
	if ((threadIdx.x & 63) == 0) {
		if (bad) atomicOr(&st->err, kIngestBadDegree);
		if (f < nf) { wave_sums[f >> 6] = s; atomicAdd(&bsum, (unsigned long long)s); }
	}
	__syncthreads();
	if (threadIdx.x < 8 && mask[threadIdx.x]) atomicOr(&st->degmask[threadIdx.x], mask[threadIdx.x]);
	if (threadIdx.x == 0 && bsum) atomicAdd(&st->total, bsum);
}

__global__ __launch_bounds__(256) void k_ingest_foff(const uint8_t *deg, uint32_t nf, const uint32_t *wave_start, uint32_t *foff)
{
	const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t s = wave_incl_scan<uint32_t>(f < nf ? deg[f] : 0);
	if (f < nf) foff[f + 1] = wave_start[f >> 6] + s;
	if (f == 0) foff[0] = 0;
}

__global__ __launch_bounds__(256) void k_ingest_foff_tri(uint32_t nf, uint32_t *foff)
{
	const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
	if (f <= nf) foff[f] = 3u * f;
}

// ---------------------------------------------------------------------------------------------------------
// indices -> org: u32 or i64 in; an index outside [0, nv) raises kIngestBadIndex and stores 0 (nothing is read at it)
// ---------------------------------------------------------------------------------------------------------
template <typename I>
__global__ __launch_bounds__(256) void k_ingest_org(const I *idx, uint32_t ne, uint32_t nv, const uint32_t *remap, uint32_t *org, IngestStatus *st)
{
	const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
	for (uint64_t h = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; h < ne; h += step) {
		const I v = idx[h];
		const bool ok = v >= 0 && (uint64_t)v < nv;
		org[h] = ok ? (remap ? remap[(uint32_t)v] : (uint32_t)v) : 0u;
		const uint64_t bad = __ballot(!ok);
		if (bad && (threadIdx.x & 63) == (uint32_t)__ffsll((unsigned long long)bad) - 1) atomicOr(&st->err, kIngestBadIndex);
	}
}

// ---------------------------------------------------------------------------------------------------------
// k_ingest_pack: record r of the output is row (rows ? rows[r] : r) of every column, byte k of a record coming from byte byte_of[k]
// of column comp_of[k].  A block writes 256 records (256 x stride bytes: a multiple of 4, so every block starts on a word), a lane
// a 4-byte word of them; the word's first record and byte take one 32-bit division.  The partial word at the end of the output is
// stored byte by byte.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_ingest_pack(PackCols p, uint32_t n, const uint32_t *rows, uint32_t nsrc, uint8_t *out)
{
	const uint32_t S = p.rec_stride;
	const uint64_t r0 = (uint64_t)blockIdx.x * 256;
	if (r0 >= n || S == 0) return;
	const uint32_t bytes = (uint32_t)min<uint64_t>(256, n - r0) * S;
	uint8_t *dst = out + r0 * S;
	for (uint32_t w = threadIdx.x; w * 4 < bytes; w += blockDim.x) {
		uint32_t rr = w * 4 / S, k = w * 4 - rr * S, word = 0;
		const uint32_t nb = min(4u, bytes - w * 4);
		for (uint32_t j = 0; j < nb; ++j) {
			const uint32_t sr = rows ? rows[r0 + rr] : (uint32_t)(r0 + rr);
			uint32_t x = 0;
			if (sr < nsrc) {
				const uint32_t c = p.comp_of[k];
				x = p.src[c][(uint64_t)sr * p.stride[c] + p.byte_of[k]];
			}
			word |= x << (8 * j);
			if (++k == S) { k = 0; ++rr; }
		}
		if (nb == 4) *(uint32_t*)(dst + w * 4) = word;
		else for (uint32_t j = 0; j < nb; ++j) dst[w * 4 + j] = (uint8_t)(word >> (8 * j));
	}
}

// ---------------------------------------------------------------------------------------------------------
// corner_attr: word 2c + s is corner c's record in the list of slot s -- its index in that list's buffer, through the list's weld
// map when welding; 0 in an unused slot.  An index outside [0, rows) raises the list's bit (one atomic per wavefront) and stores 0:
// nothing is read or written at it.
// ---------------------------------------------------------------------------------------------------------
template <typename I>
__global__ __launch_bounds__(256) void k_ingest_corner_attr(CornerSlots cs, uint32_t ne, uint32_t *cattr, IngestStatus *st)
{
	const uint64_t n = 2ull * ne, step = (uint64_t)gridDim.x * blockDim.x;
	for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < n; w += step) {
		const uint32_t s = (uint32_t)(w & 1);
		const I *idx = (const I*)cs.idx[s];
		uint32_t out = 0, raise = 0;
		if (idx) {
			const I v = idx[w >> 1];
			const bool ok = v >= 0 && (uint64_t)v < cs.rows[s];
			if (ok) out = cs.remap[s] ? cs.remap[s][(uint32_t)v] : (uint32_t)v;
			else raise = cs.bad[s];
		}
		cattr[w] = out;
		const uint64_t b0 = __ballot(raise == cs.bad[0] && raise != 0), b1 = __ballot(raise == cs.bad[1] && raise != 0);
		const uint64_t any = b0 | b1;
		if (any && (threadIdx.x & 63) == (uint32_t)__ffsll((unsigned long long)any) - 1) atomicOr(&st->err, (b0 ? cs.bad[0] : 0u) | (b1 ? cs.bad[1] : 0u));
	}
}

// ---------------------------------------------------------------------------------------------------------
// face regions: the distinct materials, numbered in order of their first face.  k_region_first: only the first face of a run of
// equal materials can be a material's first face, so only those lanes issue atomicMin(first[material], face) -- as many atomics as
// runs, and a minimum does not depend on the order they complete in.  k_region_rank (ONE block): the materials whose entry is not
// EMPTY are compacted into LDS (in any order: LDS atomic counter) and each one's region is the number of present materials with an
// earlier first face (first faces are distinct, at most 128 x 128 comparisons).  More than 128: the bit, and the count for the text.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_region_first(const uint16_t *mat, uint32_t nf, uint32_t *first)
{
	const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
	if (f >= nf) return;
	const uint16_t m = mat[f];
	if (f == 0 || mat[f - 1] != m) atomicMin(&first[m], f);
}

__global__ __launch_bounds__(256) void k_region_rank(const uint32_t *first, uint32_t *rank, uint32_t *n_regions, IngestStatus *st)
{
	__shared__ uint32_t s_n, s_mat[kIngestMaxRegions], s_first[kIngestMaxRegions];
	if (threadIdx.x == 0) s_n = 0;
	__syncthreads();
	for (uint32_t m = threadIdx.x; m < kIngestMaterials; m += blockDim.x) {
		const uint32_t f = first[m];
		if (f == kNone) continue;
		const uint32_t at = atomicAdd(&s_n, 1u);
		if (at < kIngestMaxRegions) { s_mat[at] = m; s_first[at] = f; }
	}
	__syncthreads();
	const uint32_t n = s_n, k = min(n, kIngestMaxRegions);
	if (threadIdx.x == 0) {
		*n_regions = n;
		if (n > kIngestMaxRegions) atomicOr(&st->err, kIngestManyRegions);
	}
	if (threadIdx.x < k) {
		const uint32_t mine = s_first[threadIdx.x];
		uint32_t r = 0;
		for (uint32_t j = 0; j < k; ++j) r += s_first[j] < mine;
		rank[s_mat[threadIdx.x]] = r;
	}
}

// a lane per word of face_reg (two faces); the odd face at the end is stored on its own
__global__ __launch_bounds__(256) void k_ingest_face_region(const uint16_t *mat, uint32_t nf, const uint32_t *rank, uint16_t *face_reg)
{
	const uint32_t f = 2 * (blockIdx.x * blockDim.x + threadIdx.x);
	if (f >= nf) return;
	const uint32_t a = rank[mat[f]];
	if (f + 1 < nf) ((uint32_t*)face_reg)[f >> 1] = a | rank[mat[f + 1]] << 16;
	else face_reg[f] = (uint16_t)a;
}

// ---- launchers
void launch_ingest_offsets(hipStream_t st, const uint8_t *deg, uint32_t nf, uint32_t *wave_sums, uint32_t *wave_start, uint32_t *foff, IngestStatus *status)
{
	if (!deg) {
		hipLaunchKernelGGL(k_ingest_foff_tri, dim3(((uint64_t)nf + 1 + 255) / 256), dim3(256), 0, st, nf, foff);
		return;
	}
	if (!nf) { hipLaunchKernelGGL(k_ingest_foff_tri, dim3(1), dim3(256), 0, st, 0u, foff); return; }
	const unsigned nb = (unsigned)(((uint64_t)nf + 255) / 256);
	hipLaunchKernelGGL(k_ingest_degrees, dim3(nb), dim3(256), 0, st, deg, nf, wave_sums, status);
	launch_scan_counts(st, wave_sums, (uint32_t)(((uint64_t)nf + 63) / 64), wave_start);
	hipLaunchKernelGGL(k_ingest_foff, dim3(nb), dim3(256), 0, st, deg, nf, (const uint32_t*)wave_start, foff);
}
void launch_ingest_org(hipStream_t st, const void *idx, bool idx64, uint32_t ne, uint32_t nv, const uint32_t *remap, uint32_t *org, IngestStatus *status)
{
	if (!ne) return;
	if (idx64) hipLaunchKernelGGL(k_ingest_org<int64_t>, dim3(grid_for(ne, 256)), dim3(256), 0, st, (const int64_t*)idx, ne, nv, remap, org, status);
	else hipLaunchKernelGGL(k_ingest_org<uint32_t>, dim3(grid_for(ne, 256)), dim3(256), 0, st, (const uint32_t*)idx, ne, nv, remap, org, status);
}
void launch_ingest_pack(hipStream_t st, const PackCols &p, uint32_t n, const uint32_t *rows, uint32_t nsrc, uint8_t *out)
{
	if (n && p.rec_stride) hipLaunchKernelGGL(k_ingest_pack, dim3((unsigned)(((uint64_t)n + 255) / 256)), dim3(256), 0, st, p, n, rows, nsrc, out);
}
void launch_ingest_corner_attr(hipStream_t st, const CornerSlots &cs, bool idx64, uint32_t ne, uint32_t *corner_attr, IngestStatus *status)
{
	if (!ne) return;
	if (idx64) hipLaunchKernelGGL(k_ingest_corner_attr<int64_t>, dim3(grid_for(2ull * ne, 256)), dim3(256), 0, st, cs, ne, corner_attr, status);
	else hipLaunchKernelGGL(k_ingest_corner_attr<uint32_t>, dim3(grid_for(2ull * ne, 256)), dim3(256), 0, st, cs, ne, corner_attr, status);
}
void launch_ingest_regions(hipStream_t st, const uint16_t *mat, uint32_t nf, uint32_t *first, uint32_t *rank, uint32_t *n_regions, uint16_t *face_reg,
                           IngestStatus *status)
{
	if (nf) hipLaunchKernelGGL(k_region_first, dim3((unsigned)(((uint64_t)nf + 255) / 256)), dim3(256), 0, st, mat, nf, first);
	hipLaunchKernelGGL(k_region_rank, dim3(1), dim3(256), 0, st, (const uint32_t*)first, rank, n_regions, status);
	if (nf) hipLaunchKernelGGL(k_ingest_face_region, dim3((unsigned)(((uint64_t)nf + 511) / 512)), dim3(256), 0, st, mat, nf, (const uint32_t*)rank, face_reg);
}

}   // namespace dev
}   // namespace hry
