// Per-component error of one mesh against another through a numbering map (driver: distortion.cpp; contract: include/harry_amd.h,
// hry_distortion_build).  Two kernels, wave64:
//   k_distortion_rows  a block of 256 lanes owns kDistBlockRows consecutive rows of a, lane t the rows t, t + 256, ...: consecutive
//                      lanes read consecutive map entries and records of a (coalesced) and gather one whole record of b each, so a
//                      record's components come from one cache line.  Per component the lanes' (max |e|, lowest row), sum of e*e,
//                      range of a and counters are joined over the wavefront (__shfl_down), then over the block's four wavefronts
//                      through LDS: one DistPart per block and component, and one for the positions.  The per-row buffer is written
//                      on the way.  A map entry at or above b's count raises the status word (a vector atomic, once per wavefront)
//                      and is not followed.
//   k_distortion_fold  one block per list: lane t joins its contiguous span of the blocks' records, the lanes join pairwise in
//                      LDS -- always neighbours, so everything stays in block order.
// Every join is written out in one fixed order that depends on the row count alone: no floating-point atomics, the same bits
// from run to run.  e*e is rounded on its own (-ffp-contract=off).
#include <hip/hip_runtime.h>

#include "codec_math.hpp"
#include "dequant.hpp"
#include "dev_types.hpp"
#include "fan.hpp"
#include "kernels.hpp"

namespace hry {
namespace dev {

namespace {

constexpr uint32_t kNone = 0xffffffffu;
constexpr int kLanes = 256, kWaves = kLanes / 64, kRowsPerLane = (int)(kDistBlockRows / kLanes);
static_assert(kRowsPerLane * kLanes == (int)kDistBlockRows, "a block's rows are a multiple of its lanes");

// the component's value after hry_requant(clear) -- quantised ones through dequantise_bits, the others as stored -- as a double:
// floats widen exactly, 64-bit integers round to nearest
__device__ __forceinline__ double component_f64(const uint8_t *slot, const RequantComp &c)
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
	case 0: return (double)cm::bits<float>((uint32_t)v);
	case 1: return cm::bits<double>(v);
	case 2: return (double)v;
	case 3: return (double)(int64_t)v;
	case 4: return (double)(uint32_t)v;
	case 5: return (double)(int32_t)(uint32_t)v;
	case 6: return (double)(uint16_t)v;
	case 7: return (double)(int16_t)(uint16_t)v;
	case 8: return (double)(uint8_t)v;
	case 9: return (double)(int8_t)(uint8_t)v;
	default: return 0.0;
	}
}
__device__ __forceinline__ bool finite_f64(double x) { return (cm::bits<uint64_t>(x) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull; }

template <typename P> __device__ __forceinline__ void clear(P &p)
{
	p.mx = 0.0; p.sum = 0.0; p.mn = cm::bits<double>(0x7ff0000000000000ull); p.mxa = cm::bits<double>(0xfff0000000000000ull);
	p.row = kNone; p.compared = 0; p.skipped = 0; p.nonfinite = 0; p.changed = 0;
}
// the larger maximum, between equal ones the lower row (a part without a compared pair holds (0, kNone): any compared pair beats it)
template <typename P> __device__ __forceinline__ void offer(P &p, double v, uint32_t row)
{
	if (v > p.mx || (v == p.mx && row < p.row)) { p.mx = v; p.row = row; }
}
// b's rows lie behind a's: a.sum + b.sum in that order
template <typename P, typename Q> __device__ __forceinline__ void join(P &a, const Q &b)
{
	offer(a, b.mx, b.row);
	a.sum = a.sum + b.sum;
	a.mn = b.mn < a.mn ? b.mn : a.mn;
	a.mxa = b.mxa > a.mxa ? b.mxa : a.mxa;
	a.compared += b.compared; a.skipped += b.skipped; a.nonfinite += b.nonfinite; a.changed += b.changed;
}
__device__ __forceinline__ void wave_join(DistPart &p)
{
	for (int off = 32; off > 0; off >>= 1) {   // lane 0 ends with the lanes' parts joined in a fixed tree
		DistPart o;
		o.mx = __shfl_down(p.mx, off); o.sum = __shfl_down(p.sum, off); o.mn = __shfl_down(p.mn, off); o.mxa = __shfl_down(p.mxa, off);
		o.row = __shfl_down(p.row, off); o.compared = __shfl_down(p.compared, off); o.skipped = __shfl_down(p.skipped, off);
		o.nonfinite = __shfl_down(p.nonfinite, off); o.changed = __shfl_down(p.changed, off);
		join(p, o);
	}
}

}   // namespace

__global__ __launch_bounds__(256) void k_distortion_rows(DistList L, RequantPlan pa, RequantPlan pb, uint32_t *status)
{
	__shared__ DistPart s_part[kMaxComp + 1][kWaves];
	const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
	const uint64_t base = (uint64_t)blockIdx.x * kDistBlockRows;
	const uint8_t *ra[kRowsPerLane], *rb[kRowsPerLane];
	bool live[kRowsPerLane], mapped[kRowsPerLane], pos_ok[kRowsPerLane];
	double esq[kRowsPerLane], d2[kRowsPerLane];
	uint32_t nskip = 0;
	bool bad = false;
#pragma unroll
	for (int k = 0; k < kRowsPerLane; ++k) {
		const uint64_t i = base + (uint64_t)k * kLanes + t;
		live[k] = i < L.rows;
		uint32_t j = kNone;
		if (live[k]) j = L.map ? L.map[i] : (uint32_t)i;
		if (j != kNone && j >= L.b_rows) { bad = true; j = kNone; }   // (never followed)
		mapped[k] = live[k] && j != kNone;
		nskip += live[k] && !mapped[k];
		ra[k] = L.a + (mapped[k] ? i : 0) * L.sa;
		rb[k] = L.b + (size_t)(mapped[k] ? j : 0) * L.sb;
		pos_ok[k] = mapped[k];
		esq[k] = 0.0; d2[k] = 0.0;
	}
	const uint64_t any_bad = __ballot(bad);
	if (any_bad && lane == (uint32_t)__ffsll((unsigned long long)any_bad) - 1) atomicOr(status, 1u);

	for (int c = 0; c < pa.n; ++c) {
		const RequantComp &ca = pa.c[c], &cb = pb.c[c];
		const bool is_pos = L.pos >= 0 && c >= L.pos && c < L.pos + 3;
		DistPart p;
		clear(p);
		p.skipped = nskip;
#pragma unroll
		for (int k = 0; k < kRowsPerLane; ++k) {
			if (!mapped[k]) continue;
			const double x = component_f64(ra[k] + ca.off, ca), y = component_f64(rb[k] + cb.off, cb);
			if (finite_f64(x) && finite_f64(y)) {
				const double e = y - x, sq = e * e;
				offer(p, fabs(e), (uint32_t)(base + (uint64_t)k * kLanes + t));
				p.sum = p.sum + sq;
				p.mn = x < p.mn ? x : p.mn;
				p.mxa = x > p.mxa ? x : p.mxa;
				p.compared += 1;
				p.changed += e != 0.0;
				esq[k] = esq[k] + sq;
				if (is_pos) d2[k] = c == L.pos ? sq : d2[k] + sq;   // (ex*ex + ey*ey) + ez*ez
			} else {
				p.nonfinite += 1;
				p.changed += cm::bits<uint64_t>(x) != cm::bits<uint64_t>(y);
				if (is_pos) pos_ok[k] = false;
			}
		}
		wave_join(p);
		if (lane == 0) s_part[c][wave] = p;
	}
	if (L.pos >= 0) {
		DistPart p;
		clear(p);
		p.skipped = nskip;
#pragma unroll
		for (int k = 0; k < kRowsPerLane; ++k) {
			if (!pos_ok[k]) continue;
			offer(p, sqrt(d2[k]), (uint32_t)(base + (uint64_t)k * kLanes + t));
			p.sum = p.sum + d2[k];
			p.compared += 1;
		}
		wave_join(p);
		if (lane == 0) s_part[pa.n][wave] = p;
	}
	if (L.err) {
#pragma unroll
		for (int k = 0; k < kRowsPerLane; ++k)
			if (live[k]) L.err[base + (uint64_t)k * kLanes + t] = mapped[k] ? (float)sqrt(esq[k]) : 0.0f;
	}
	__syncthreads();
	const uint32_t nslots = (uint32_t)pa.n + (L.pos >= 0 ? 1u : 0u);
	if (t < nslots) {
		DistPart p = s_part[t][0];
		for (int w = 1; w < kWaves; ++w) join(p, s_part[t][w]);
		p.pad[0] = p.pad[1] = p.pad[2] = 0;
		L.part[(size_t)blockIdx.x * nslots + t] = p;
	}
}

__global__ __launch_bounds__(256) void k_distortion_fold(DistFold f, DistFinal *out)
{
	__shared__ DistFinal s[kLanes];
	const uint32_t t = threadIdx.x, l = blockIdx.x;
	const DistPart *part = f.part[l];
	const uint32_t nb = f.nblocks[l], ns = f.nslots[l];
	const uint32_t per = (nb + kLanes - 1) / kLanes;
	const uint32_t b0 = min(nb, t * per), b1 = min(nb, b0 + per);   // (nb < 2^22: t * per stays below 2^32)
	for (uint32_t c = 0; c < ns; ++c) {
		DistFinal a;
		clear(a);
		a.reserved = 0;
		for (uint32_t b = b0; b < b1; ++b) join(a, part[(size_t)b * ns + c]);
		s[t] = a;
		__syncthreads();
		for (uint32_t d = 1; d < (uint32_t)kLanes; d <<= 1) {
			if ((t & (2 * d - 1)) == 0) join(s[t], s[t + d]);
			__syncthreads();
		}
		if (t == 0) out[f.out_at[l] + c] = s[0];
		__syncthreads();
	}
}

void launch_distortion_rows(hipStream_t st, const DistList &L, const RequantPlan &pa, const RequantPlan &pb, uint32_t *status)
{
	if (L.rows) hipLaunchKernelGGL(k_distortion_rows, dim3(distortion_blocks(L.rows)), dim3(kLanes), 0, st, L, pa, pb, status);
}
void launch_distortion_fold(hipStream_t st, const DistFold &f, DistFinal *out)
{
	if (f.n > 0) hipLaunchKernelGGL(k_distortion_fold, dim3((unsigned)f.n), dim3(kLanes), 0, st, f, out);
}

}   // namespace dev
}   // namespace hry
