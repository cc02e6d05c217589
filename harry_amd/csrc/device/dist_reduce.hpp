// The error statistics of hry_comp_error on the device, shared by k_distortion_rows / k_distortion_fold (distortion.hip) and
// k_quant_sweep / k_quant_sweep_fold (sweep.hip): a value as a double, one pair into a lane's record, the joins of lanes,
// wavefronts and blocks.  Every join is written out in one fixed order: no floating-point atomics, the same bits from run to run.
// The joins are templates over the record: DistPart / DistFinal, and their siblings for the faces' normal deviation, NormPart /
// NormFinal (normal_sweep.hip) -- a record type brings its own clear, join, shuffled and tidy.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "codec_math.hpp"
#include "dev_types.hpp"

namespace hry {
namespace dev {

constexpr uint32_t kDistNone = 0xffffffffu;

using cm::value_f64;   // a component's raw bits as a double (codec_math.hpp)
__device__ __forceinline__ bool finite_f64(double x) { return (cm::bits<uint64_t>(x) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull; }

template <typename P> __device__ __forceinline__ void clear(P &p)
{
	p.mx = 0.0; p.sum = 0.0; p.mn = cm::bits<double>(0x7ff0000000000000ull); p.mxa = cm::bits<double>(0xfff0000000000000ull);
	p.row = kDistNone; p.compared = 0; p.skipped = 0; p.nonfinite = 0; p.changed = 0;
}
// the larger maximum, between equal ones the lower row (a part without a compared pair holds (0, kDistNone): any compared pair beats it)
template <typename P> __device__ __forceinline__ void offer(P &p, double v, uint32_t row)
{
	if (v > p.mx || (v == p.mx && row < p.row)) { p.mx = v; p.row = row; }
}
// the pair (x of a, y of b) of row `row` into a lane's record.  true: both finite, the pair is compared and sq = e*e (rounded on
// its own); false: it counts in nonfinite
__device__ __forceinline__ bool tally(DistPart &p, double x, double y, uint32_t row, double &sq)
{
	if (finite_f64(x) && finite_f64(y)) {
		const double e = y - x;
		sq = e * e;
		offer(p, fabs(e), row);
		p.sum = p.sum + sq;
		p.mn = x < p.mn ? x : p.mn;
		p.mxa = x > p.mxa ? x : p.mxa;
		p.compared += 1;
		p.changed += e != 0.0;
		return true;
	}
	p.nonfinite += 1;
	p.changed += cm::bits<uint64_t>(x) != cm::bits<uint64_t>(y);
	return false;
}
__device__ __forceinline__ void clear(NormPart &p) { p.mx = 0.0; p.sum = 0.0; p.row = kDistNone; p.compared = 0; p.skipped = 0; p.nonfinite = 0; p.degenerate = 0; p.collapsed = 0; }
__device__ __forceinline__ void clear(NormFinal &p) { p.mx = 0.0; p.sum = 0.0; p.row = kDistNone; p.compared = 0; p.skipped = 0; p.nonfinite = 0; p.degenerate = 0; p.collapsed = 0; }
// b's rows lie behind a's: a.sum + b.sum in that order
template <typename P, typename Q> __device__ __forceinline__ void join_normals(P &a, const Q &b)
{
	offer(a, b.mx, b.row);
	a.sum = a.sum + b.sum;
	a.compared += b.compared; a.skipped += b.skipped; a.nonfinite += b.nonfinite; a.degenerate += b.degenerate; a.collapsed += b.collapsed;
}
template <typename Q> __device__ __forceinline__ void join(NormPart &a, const Q &b) { join_normals(a, b); }
template <typename Q> __device__ __forceinline__ void join(NormFinal &a, const Q &b) { join_normals(a, b); }
template <typename P, typename Q> __device__ __forceinline__ void join(P &a, const Q &b)
{
	offer(a, b.mx, b.row);
	a.sum = a.sum + b.sum;
	a.mn = b.mn < a.mn ? b.mn : a.mn;
	a.mxa = b.mxa > a.mxa ? b.mxa : a.mxa;
	a.compared += b.compared; a.skipped += b.skipped; a.nonfinite += b.nonfinite; a.changed += b.changed;
}
// the record of the lane `off` lanes up
__device__ __forceinline__ DistPart shuffled(const DistPart &p, int off)
{
	DistPart o;
	o.mx = __shfl_down(p.mx, off); o.sum = __shfl_down(p.sum, off); o.mn = __shfl_down(p.mn, off); o.mxa = __shfl_down(p.mxa, off);
	o.row = __shfl_down(p.row, off); o.compared = __shfl_down(p.compared, off); o.skipped = __shfl_down(p.skipped, off);
	o.nonfinite = __shfl_down(p.nonfinite, off); o.changed = __shfl_down(p.changed, off);
	return o;
}
__device__ __forceinline__ NormPart shuffled(const NormPart &p, int off)
{
	NormPart o;
	o.mx = __shfl_down(p.mx, off); o.sum = __shfl_down(p.sum, off);
	o.row = __shfl_down(p.row, off); o.compared = __shfl_down(p.compared, off); o.skipped = __shfl_down(p.skipped, off);
	o.nonfinite = __shfl_down(p.nonfinite, off); o.degenerate = __shfl_down(p.degenerate, off); o.collapsed = __shfl_down(p.collapsed, off);
	return o;
}
// what a record's padding holds where it is stored
__device__ __forceinline__ void tidy(DistPart &p) { p.pad[0] = p.pad[1] = p.pad[2] = 0; }
__device__ __forceinline__ void tidy(NormPart &p) { p.pad[0] = p.pad[1] = 0; }
__device__ __forceinline__ void tidy(DistFinal &p) { p.reserved = 0; }
__device__ __forceinline__ void tidy(NormFinal &p) { p.list = 0; }
template <typename P> __device__ __forceinline__ void wave_join(P &p)
{
	for (int off = 32; off > 0; off >>= 1) {   // lane 0 ends with the lanes' parts joined in a fixed tree
		const P o = shuffled(p, off);
		join(p, o);
	}
}
// the wavefronts' records of one slot (LDS, kWaves of them) joined in wavefront order, as a block leaves it
template <int kWaves, typename P> __device__ __forceinline__ P block_join(const P *s)
{
	P p = s[0];
	for (int w = 1; w < kWaves; ++w) join(p, s[w]);
	tidy(p);
	return p;
}
// one slot of nb blocks' records (block b's at part[b * ns + c]) into *out, by a whole block of kLanes lanes: lane t joins its
// contiguous span of the blocks, the lanes join pairwise in LDS (s: kLanes records) -- always neighbours, so everything stays in
// block order.  Ends behind a barrier: s may be used again at once
template <int kLanes, typename P, typename F> __device__ __forceinline__ void fold_slot(const P *part, uint32_t nb, uint32_t ns, uint32_t c, F *s, F *out)
{
	const uint32_t t = threadIdx.x;
	const uint32_t per = (nb + kLanes - 1) / kLanes;
	const uint32_t b0 = min(nb, t * per), b1 = min(nb, b0 + per);   // (nb < 2^22: t * per stays below 2^32)
	F a;
	clear(a);
	tidy(a);
	for (uint32_t b = b0; b < b1; ++b) join(a, part[(size_t)b * ns + c]);
	s[t] = a;
	__syncthreads();
	for (uint32_t d = 1; d < (uint32_t)kLanes; d <<= 1) {
		if ((t & (2 * d - 1)) == 0) join(s[t], s[t + d]);
		__syncthreads();
	}
	if (t == 0) *out = s[0];
	__syncthreads();
}

}   // namespace dev
}   // namespace hry
