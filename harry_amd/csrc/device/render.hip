// Render-ready device buffers of a mesh (driver: render.cpp; contract: include/harry_amd.h, hry_render_build).  Streaming
// kernels, wave64, one element per lane and consecutive lanes on consecutive output words (coalesced stores):
//   k_tri_face       fan triangulation, a face per lane: the source face of each of its deg - 2 triangles
//   k_fan_indices    a lane per index WORD (3 per triangle): corner c0 / c(k+1) / c(k+2) of its triangle, through the vertex map
//   k_rows_of        the record every output row names in one list (general bindings)
//   k_render_gather  a lane per f32 of a list's output: the component's value, dequantised (dequant.hpp), as float
//   k_place_*        a decoded segment of a sharded container into the whole mesh's numbering
// The unweld of general bindings with corner lists (one output vertex per distinct corner key) is dedup.hip's numbering over an
// UnweldView's keys; the identity vertex_source is its k_iota.
#include <hip/hip_runtime.h>

#include "codec_math.hpp"
#include "dequant.hpp"
#include "dev_types.hpp"
#include "fan.hpp"
#include "kernels.hpp"

namespace hry {
namespace dev {

constexpr uint32_t kNone = 0xffffffffu;

// ---------------------------------------------------------------------------------------------------------
// fan triangulation (structs/conn.h:87: T = sum(deg - 2)); triangle k of face f is (c0, c(k+1), c(k+2)); the first triangle
// of face f is foff[f] - 2f.  Every index is bounds-checked against the sizes the host passes: even a face with fewer than three
// corners (no reader or constructor builds one) could not make a lane write outside the buffers.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_tri_face(const uint32_t *foff, uint32_t nf, uint64_t ntri, uint32_t *tri_face)
{
	const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
	if (f >= nf) return;
	const uint32_t lo = foff[f], hi = foff[f + 1];
	if (hi < lo + 3) return;
	const uint64_t t0 = (uint64_t)lo - 2ull * f;
	const uint32_t n = hi - lo - 2;   // a face of any degree: its lane loops (coded meshes: at most 127 triangles)
	for (uint32_t k = 0; k < n; ++k)
		if (t0 + k < ntri) tri_face[t0 + k] = f;
}

__global__ __launch_bounds__(256) void k_fan_indices(const uint32_t *foff, uint32_t nf, const uint32_t *tri_face, const uint32_t *vmap, uint32_t ne,
                                                     uint64_t nwords, uint32_t *out)
{
	const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
	for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < nwords; w += step) {
		const uint64_t t = w / 3;
		const uint32_t j = (uint32_t)(w - t * 3);
		const uint32_t f = tri_face[t];
		uint32_t v = 0;
		if (f < nf) {
			const uint32_t lo = foff[f];
			const uint64_t k = t - ((uint64_t)lo - 2ull * f);
			const uint64_t c = j == 0 ? (uint64_t)lo : (uint64_t)lo + k + j;
			if (c < ne) v = vmap[c];
		}
		out[w] = v;
	}
}

// ---------------------------------------------------------------------------------------------------------
// rows -> records of one list (general bindings): element e of row u (src[u], or u), the region of e (or of its face: efc),
// the slot the region binds the list at; kNone where it binds none or the record is out of range
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_rows_of(RowsView v, uint32_t rows, uint32_t *idx)
{
	const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
	if (u >= rows) return;
	const uint32_t e = v.src ? v.src[u] : u;
	uint32_t rec = kNone;
	if (e < v.nelem) {
		const uint32_t owner = v.efc ? v.efc[e] : e;
		const uint32_t r = owner < v.nowner ? v.reg[owner] : kNone;
		const int32_t s = r < v.nregs ? v.slot[r] : -1;
		if (s >= 0) rec = v.attr[(size_t)e * v.nb + (uint32_t)s];
	}
	idx[u] = rec < v.count ? rec : kNone;
}

// ---------------------------------------------------------------------------------------------------------
// k_render_gather: out[row * n + k] = (float) of component k of the record of `row` after hry_requant(clear): quantised
// components through dequantise_bits (the formula k_requant applies in place), the others as they are; lossless floats bit
// for bit.  Rows without a record (idx == kNone) get 0.
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float component_f32(const uint8_t *slot, const RequantComp &c)
{
	uint64_t v;
	if (c.src_bits) {
		uint64_t q;
		switch (c.src_type) {   // storage type of the quantised value (quant.h:121-129)
		case 8: q = ldg<uint8_t>(slot); break;
		case 6: q = ldg<uint16_t>(slot); break;
		case 4: q = ldg<uint32_t>(slot); break;
		default: q = ldg<uint64_t>(slot); break;
		}
		v = dequantise_bits(q, c);
	} else {
		switch (c.dst_type) {
		case 1: case 2: case 3: v = ldg<uint64_t>(slot); break;
		case 6: case 7: v = ldg<uint16_t>(slot); break;
		case 8: case 9: v = ldg<uint8_t>(slot); break;
		default: v = ldg<uint32_t>(slot); break;
		}
	}
	switch (c.dst_type) {
	case 0: return cm::bits<float>((uint32_t)v);
	case 1: return (float)cm::bits<double>(v);
	case 2: return (float)v;
	case 3: return (float)(int64_t)v;
	case 4: return (float)(uint32_t)v;
	case 5: return (float)(int32_t)(uint32_t)v;
	case 6: return (float)(uint16_t)v;
	case 7: return (float)(int16_t)(uint16_t)v;
	case 8: return (float)(uint8_t)v;
	case 9: return (float)(int8_t)(uint8_t)v;
	default: return 0.0f;
	}
}

__global__ __launch_bounds__(256) void k_render_gather(const uint8_t *rec, int stride, uint32_t count, const uint32_t *idx, uint64_t rows, RequantPlan plan, float *out)
{
	const uint64_t total = rows * (uint64_t)plan.n, step = (uint64_t)gridDim.x * blockDim.x;
	for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < total; w += step) {
		const uint64_t row = w / (uint32_t)plan.n;
		const int k = (int)(w - row * (uint32_t)plan.n);
		const uint32_t r = idx ? idx[row] : (uint32_t)row;
		float x = 0.0f;
		if (r < count) x = component_f32(rec + (size_t)r * stride + plan.c[k].off, plan.c[k]);
		out[w] = x;
	}
}

// ---------------------------------------------------------------------------------------------------------
// placement of a decoded segment of a sharded container (.hry v0.3, decoded on one context) into the whole mesh's numbering: the
// runs of the segment lie back to back in its own numbering (local first element l*[j]) and at g*[j] in the whole one.  Element i
// of a kind belongs to the last run j with l[j] <= i (empty runs are skipped that way).
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t run_of(const uint32_t *l, uint32_t nr, uint32_t i)
{
	uint32_t lo = 0, hi = nr;
	while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (l[mid] <= i) lo = mid; else hi = mid; }
	return lo;
}
__global__ __launch_bounds__(256) void k_place_records(const uint8_t *src, uint32_t n, uint32_t stride, const uint32_t *l, const uint32_t *g, uint32_t nr, uint32_t gn, uint8_t *dst)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const uint32_t j = run_of(l, nr, i), gi = g[j] + (i - l[j]);
	if (gi >= gn) return;
	const uint8_t *a = src + (size_t)i * stride;
	uint8_t *b = dst + (size_t)gi * stride;
	for (uint32_t k = 0; k < stride; ++k) b[k] = a[k];
}
__global__ __launch_bounds__(256) void k_place_org(RunPlace r, const uint32_t *org, uint32_t ne, uint32_t *dst)
{
	const uint32_t h = blockIdx.x * blockDim.x + threadIdx.x;
	if (h >= ne) return;
	const uint32_t j = run_of(r.lh, r.nr, h), gh = r.gh[j] + (h - r.lh[j]);
	const uint32_t v = org[h], jv = run_of(r.lv, r.nr, v), gv = r.gv[jv] + (v - r.lv[jv]);
	if (gh < r.gne) dst[gh] = gv < r.gnv ? gv : 0;
}
__global__ __launch_bounds__(256) void k_place_foff(RunPlace r, const uint32_t *foff, uint32_t nf, uint32_t *dst)
{
	const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
	if (f >= nf) return;
	const uint32_t j = run_of(r.lf, r.nr, f), gf = r.gf[j] + (f - r.lf[j]);
	if (gf >= r.gnf) return;
	const uint32_t shift = r.gh[j] - r.lh[j];   // modulo 2^32: local half-edge + shift = half-edge of the whole mesh
	if (f == r.lf[j]) dst[gf] = r.gh[j];
	dst[gf + 1] = foff[f + 1] + shift;
}

// ---- launchers
void launch_fan(hipStream_t st, const uint32_t *foff, uint32_t nf, uint64_t ntri, const uint32_t *vmap, uint32_t ne, uint32_t *tri_face, uint32_t *indices)
{
	if (!nf || !ntri) return;
	hipLaunchKernelGGL(k_tri_face, dim3((nf + 255) / 256), dim3(256), 0, st, foff, nf, ntri, tri_face);
	hipLaunchKernelGGL(k_fan_indices, dim3(grid_for(3 * ntri, 256)), dim3(256), 0, st, foff, nf, (const uint32_t*)tri_face, vmap, ne, 3 * ntri, indices);
}
void launch_rows_of(hipStream_t st, const RowsView &v, uint32_t rows, uint32_t *idx)
{
	if (rows) hipLaunchKernelGGL(k_rows_of, dim3((rows + 255) / 256), dim3(256), 0, st, v, rows, idx);
}
void launch_place_segment(hipStream_t st, const RunPlace &r, const uint8_t *vrec, uint32_t nlv, uint32_t vstride, uint8_t *whole_vrec,
                          const uint8_t *frec, uint32_t nlf, uint32_t fstride, uint8_t *whole_frec, const uint32_t *org, uint32_t nle, uint32_t *whole_org,
                          const uint32_t *foff, uint32_t *whole_foff)
{
	if (!r.nr) return;
	if (nlv && vstride) hipLaunchKernelGGL(k_place_records, dim3((nlv + 255) / 256), dim3(256), 0, st, vrec, nlv, vstride, r.lv, r.gv, r.nr, r.gnv, whole_vrec);
	if (nlf && fstride) hipLaunchKernelGGL(k_place_records, dim3((nlf + 255) / 256), dim3(256), 0, st, frec, nlf, fstride, r.lf, r.gf, r.nr, r.gnf, whole_frec);
	if (nle) hipLaunchKernelGGL(k_place_org, dim3((nle + 255) / 256), dim3(256), 0, st, r, org, nle, whole_org);
	if (nlf) hipLaunchKernelGGL(k_place_foff, dim3((nlf + 255) / 256), dim3(256), 0, st, r, foff, nlf, whole_foff);
}
void launch_render_gather(hipStream_t st, const uint8_t *rec, int stride, uint32_t count, const uint32_t *idx, uint64_t rows, const RequantPlan &plan, float *out)
{
	if (rows && plan.n) hipLaunchKernelGGL(k_render_gather, dim3(grid_for(rows * (uint64_t)plan.n, 256)), dim3(256), 0, st, rec, stride, count, idx, rows, plan, out);
}

}   // namespace dev
}   // namespace hry
