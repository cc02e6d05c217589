// The hierarchy over the triangles of a render build, built where the render build lies in HBM, and the ray cast and the closest-
// point query over it (include/harry_amd.h: hry_bvh_build, hry_bvh_cast, hry_bvh_nearest; kernels: bvh.hip; DESIGN.md "Bvh").  The
// build uploads nothing: it reads the render result's indices and the float rows of its position list; sixty-four bytes come down
// between its two stretches (the number of leaves sizes the buffers, the depth counts the launches of the box fit).  The result
// keeps its own copy of the leaves' positions, so the render build may be freed.  The decode's token and the encoder's resident
// mesh are left alone.  The two queries share their checks and the staging of host arrays (QueryArrays, check_query, run_query).
// The pairs of triangles that pass through each other (hry_intersections_build) are a build of their own over the hierarchy alone.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "result_build.hpp"

namespace hry {

using namespace dev;

void bvh_build(Context &cx, const Mesh &m, const RenderResult &r, uint32_t flags, BvhResult &out)
{
	if (flags) throw Error(HRY_E_ARG, "unknown bvh flag");
	require_render_of(cx, m, r);
	const uint32_t T = (uint32_t)m.ntri();
	BvhWork w{};
	w.indices = r.ptr<const uint32_t>("indices"); w.T = T; w.nout = r.nverts;
	w.pos = render_positions(m, r, "bvh", w.pos_stride);
	HIP_OK(hipSetDevice(cx.device));

	// ---- the working buffer (BvhWork, dev_types.hpp)
	Carve W;
	W.take(w.flag, (size_t)T * 4); W.take(w.at, ((size_t)T + 1) * 4); W.take(w.code_a, (size_t)T * 4); W.take(w.tri_a, (size_t)T * 4);
	W.take(w.code_b, (size_t)T * 4); W.take(w.tri_b, (size_t)T * 4); W.take(w.children, (size_t)T * 8); W.take(w.leaf_parent, (size_t)T * 4);
	W.take(w.node_parent, (size_t)T * 4); W.take(w.sums, scan_sums_words(T) * 4); W.take(w.radix, bvh_radix_words(T) * 4); W.take(w.words, 64);
	cx.d_bvh.ensure(W.total);
	W.bind(cx.d_bvh.p);

	hipStream_t st = cx.stream;
	StretchTimer timer;
	timer.mark(st);
	launch_bvh_first(st, w);
	timer.mark(st);
	uint32_t words[16] = {};
	HIP_OK(hipMemcpyAsync(words, w.words, 64, hipMemcpyDeviceToHost, st));
	HIP_OK(hipStreamSynchronize(st));
	const uint32_t L = words[0], distinct = words[1], depth = words[2];
	// every level consumes at least one of the key's 62 significant bits (30 of the code, 32 of the leaf's number): the cast's stack
	// of 64 entries rests on this
	if (L > T || depth > 62) throw Error(HRY_E_INTERNAL, "bvh: the tree is deeper than its keys allow");

	// ---- the outputs, in one allocation
	const uint64_t nodes = L ? L - 1 : 0;
	OutputPlan plan;
	plan.add("leaf_tri", L, 1, HRY_UINT);
	plan.add("leaf_code", L, 1, HRY_UINT);
	plan.add("leaf_box", L, 6, HRY_FLOAT);
	plan.add("leaf_positions", L, 9, HRY_FLOAT);
	plan.add("node_children", nodes, 2, HRY_UINT);
	plan.add("node_box", nodes, 6, HRY_FLOAT);
	plan.add("scene_box", 1, 6, HRY_FLOAT);
	plan.alloc(cx.device, out);
	const BvhView v = bvh_view_of(out);

	timer.mark(st);
	launch_bvh_second(st, w, v, depth);
	timer.mark(st);
	HIP_OK(hipStreamSynchronize(st));
	out.device_ms = timer.ms();
	out.uploaded_bytes = 0;
	out.summary[0] = T; out.summary[1] = L; out.summary[2] = (uint64_t)T - L; out.summary[3] = distinct; out.summary[4] = depth; out.summary[5] = 0;
}

BvhView bvh_view_of(const BvhResult &b)
{
	return BvhView{ (uint32_t)b.find("leaf_tri")->rows, b.ptr<uint32_t>("leaf_tri"), b.ptr<uint32_t>("leaf_code"), b.ptr<uint32_t>("node_children"), b.ptr<float>("leaf_box"),
	                b.ptr<float>("leaf_positions"), b.ptr<float>("node_box"), b.ptr<float>("scene_box") };
}

namespace {

// memory the caller calls host memory: anything the runtime does not know as device memory
void check_host_memory(const void *p, const char *what, const char *call)
{
	hipPointerAttribute_t a{};
	const hipError_t e = hipPointerGetAttributes(&a, p);
	if (e != hipSuccess) { (void)hipGetLastError(); return; }
	if (a.type == hipMemoryTypeDevice) throw Error(HRY_E_ARG, std::string(what) + ": device memory in " + call);
}

// The caller's arrays of one query against a hierarchy (a cast, a closest-point query): what both check of them and how both stage
// them.  Without the host flag every array is memory of cx's device and the kernel reads and writes it where it lies; with it
// every array is host memory and has a piece of cx.d_bvh, filled before the kernel (inputs) or copied back behind it (outputs).
// An optional array the caller left out is null on both sides.
struct QueryArrays {
	struct Item { const void *user; uint64_t bytes, align; const char *name; bool output; uint8_t *staged; };
	const char *what, *host_call;   // "cast", "a cast with HRY_CAST_HOST"
	bool host;
	std::vector<Item> items;   // complete before take(): the pieces are bound where the items lie
	void add(const void *user, uint64_t bytes, const char *name, bool output, uint64_t align = 4) { items.push_back(Item{ user, bytes, align, name, output, nullptr }); }
	// every pointer aligned, and what the flags say it is; selects cx's device
	void check(Context &cx) const
	{
		for (const Item &i : items)
			if ((uintptr_t)i.user % i.align) throw Error(HRY_E_ARG, std::string(what) + ": a misaligned pointer");
		HIP_OK(hipSetDevice(cx.device));
		for (const Item &i : items) {
			if (!i.user) continue;
			if (host) check_host_memory(i.user, i.name, host_call);
			else check_device_memory(cx, i.user, i.bytes, i.name);
		}
	}
	void take(Carve &W) { for (Item &i : items) W.take(i.staged, host && i.user ? i.bytes : 0); }
	template <typename T> T *dev(size_t k) const { const Item &i = items[k]; return (T*)(!i.user ? nullptr : host ? i.staged : (uint8_t*)i.user); }
	void upload(hipStream_t st) const
	{
		if (!host) return;
		for (const Item &i : items) if (i.user && !i.output) HIP_OK(hipMemcpyAsync(i.staged, i.user, i.bytes, hipMemcpyHostToDevice, st));
	}
	void download(hipStream_t st) const
	{
		if (!host) return;
		for (const Item &i : items) if (i.user && i.output) HIP_OK(hipMemcpyAsync((void*)i.user, i.staged, i.bytes, hipMemcpyDeviceToHost, st));
	}
};

// the refusals a query makes before it looks at its arrays
void check_query(const Context &cx, const BvhResult &b, uint32_t flags, uint32_t known, uint64_t stride_bits, const char *what)
{
	if (flags & ~known) throw Error(HRY_E_ARG, std::string("unknown ") + what + " flag");
	if (stride_bits % 4) throw Error(HRY_E_ARG, std::string(what) + ": a stride is not a multiple of 4");
	if (b.block.device != cx.device) throw Error(HRY_E_ARG, "the hierarchy lives on another device than the context's");
}

// the kernel between two marks, the counters down, the staged results back: returns the kernel's milliseconds
template <typename Launch>
double run_query(Context &cx, const QueryArrays &io, unsigned long long *d_stat, unsigned long long *counters, size_t words, Launch launch)
{
	hipStream_t st = cx.stream;
	io.upload(st);
	HIP_OK(hipMemsetAsync(d_stat, 0, words * 8, st));
	StretchTimer timer;
	timer.mark(st);
	launch(st);
	timer.mark(st);   // (one stretch)
	HIP_OK(hipMemcpyAsync(counters, d_stat, words * 8, hipMemcpyDeviceToHost, st));
	io.download(st);
	HIP_OK(hipStreamSynchronize(st));
	return timer.ms();
}

}   // namespace

void bvh_cast(Context &cx, const BvhResult &b, uint64_t n, const float *origins, uint64_t origin_stride, const float *dirs, uint64_t dir_stride, double tmin, double tmax,
              uint32_t flags, uint32_t *hit_tri, float *hit_t, float *hit_uv, uint64_t *stat, double *device_ms)
{
	check_query(cx, b, flags, HRY_CAST_HOST, origin_stride | dir_stride, "cast");
	if (std::isnan(tmin) || std::isnan(tmax)) throw Error(HRY_E_ARG, "cast: tmin or tmax is NaN");
	if (stat) stat[0] = stat[1] = 0;
	if (device_ms) *device_ms = 0.0;
	if (!n) return;
	if (n > (1ull << 40) / std::max<uint64_t>(std::max(origin_stride, dir_stride), 12)) throw Error(HRY_E_UNSUPPORTED, "cast: more than 2^40 bytes of rays");
	QueryArrays io{ "cast", "a cast with HRY_CAST_HOST", (flags & HRY_CAST_HOST) != 0, {} };
	io.add(origins, (n - 1) * origin_stride + 12, "origins", false); io.add(dirs, (n - 1) * dir_stride + 12, "dirs", false);
	io.add(hit_tri, n * 4, "hit_tri", true); io.add(hit_t, n * 4, "hit_t", true); io.add(hit_uv, n * 8, "hit_uv", true);
	io.check(cx);

	// ---- the working buffer: the two counters; with HRY_CAST_HOST the staged rays and results behind them
	Carve W;
	BvhCast c{};
	c.n = n; c.o_stride = origin_stride; c.d_stride = dir_stride; c.tmin = tmin; c.tmax = tmax;
	W.take(c.stat, 16);
	io.take(W);
	cx.d_bvh.ensure(W.total);
	W.bind(cx.d_bvh.p);
	c.o = io.dev<const uint8_t>(0); c.d = io.dev<const uint8_t>(1); c.hit_tri = io.dev<uint32_t>(2); c.hit_t = io.dev<float>(3); c.hit_uv = io.dev<float>(4);
	unsigned long long counters[2] = {};
	const double ms = run_query(cx, io, c.stat, counters, 2, [&](hipStream_t st) { launch_bvh_cast(st, bvh_view_of(b), c); });
	if (stat) { stat[0] = counters[0]; stat[1] = counters[1]; }
	if (device_ms) *device_ms = ms;
}

void bvh_nearest(Context &cx, const BvhResult &b, uint64_t n, const float *points, uint64_t point_stride, double max_dist, uint32_t flags, uint32_t *near_tri,
                 double *near_d2, float *near_uv, float *near_point, uint64_t *stat, double *device_ms)
{
	check_query(cx, b, flags, HRY_NEAREST_HOST, point_stride, "nearest");
	if (std::isnan(max_dist)) throw Error(HRY_E_ARG, "nearest: max_dist is NaN");
	if (!n) {
		if (stat) stat[0] = stat[1] = stat[2] = 0;
		if (device_ms) *device_ms = 0.0;
		return;
	}
	if (n > (1ull << 40) / std::max<uint64_t>(point_stride, 12)) throw Error(HRY_E_UNSUPPORTED, "nearest: more than 2^40 bytes of points");
	QueryArrays io{ "nearest", "a closest-point query with HRY_NEAREST_HOST", (flags & HRY_NEAREST_HOST) != 0, {} };
	io.add(points, (n - 1) * point_stride + 12, "points", false); io.add(near_tri, n * 4, "near_tri", true); io.add(near_d2, n * 8, "near_d2", true, 8);
	io.add(near_uv, n * 8, "near_uv", true); io.add(near_point, n * 12, "near_point", true);
	io.check(cx);

	// ---- the working buffer: the three counters; with HRY_NEAREST_HOST the staged points and results behind them
	Carve W;
	BvhNearest c{};
	c.n = n; c.q_stride = point_stride; c.r2 = max_dist * max_dist; c.any = max_dist < 0.0 ? 0u : 1u;
	W.take(c.stat, 24);
	io.take(W);
	cx.d_bvh.ensure(W.total);
	W.bind(cx.d_bvh.p);
	c.q = io.dev<const uint8_t>(0); c.near_tri = io.dev<uint32_t>(1); c.near_d2 = io.dev<double>(2); c.near_uv = io.dev<float>(3); c.near_point = io.dev<float>(4);
	unsigned long long counters[3] = {};
	const double ms = run_query(cx, io, c.stat, counters, 3, [&](hipStream_t st) { launch_bvh_nearest(st, bvh_view_of(b), c); });
	if (stat) { stat[0] = counters[0]; stat[1] = counters[1]; stat[2] = counters[2]; }
	if (device_ms) *device_ms = ms;
}

// The third query has a result of a size nobody knows beforehand, so it is a build in two stretches: the walk counts, sixty-four
// bytes come down (C, N, the box tests and P; the scan's P and H behind them), the outputs are allocated, the same walk fills.  It
// reads the hierarchy alone
void intersections_build(Context &cx, const BvhResult &b, uint32_t flags, IntersectionsResult &out)
{
	if (flags) throw Error(HRY_E_ARG, "unknown intersections flag");
	if (b.block.device != cx.device) throw Error(HRY_E_ARG, "the hierarchy lives on another device than the context's");
	const BvhView v = bvh_view_of(b);
	const uint32_t T = (uint32_t)b.summary[0], L = v.L;
	HIP_OK(hipSetDevice(cx.device));

	// ---- the working buffer of the first stretch: the eight words that come down, the leaves' counts and their scan
	Carve W;
	BvhPairs c{};
	uint32_t *sums, *key_b = nullptr, *val_b = nullptr, *radix = nullptr;
	c.T = T;
	W.take(c.stat, 64); W.take(c.count, (size_t)L * 4); W.take(c.start, ((size_t)L + 1) * 4); W.take(sums, scan_sums_words(L) * 4);
	const size_t first = W.total;
	cx.d_bvh.ensure(first);
	W.bind(cx.d_bvh.p);
	c.words = (uint32_t*)(c.stat + 4);

	hipStream_t st = cx.stream;
	HIP_OK(hipMemsetAsync(c.stat, 0, 64, st));
	StretchTimer timer;
	timer.mark(st);
	launch_bvh_pairs_count(st, v, c, sums);
	timer.mark(st);
	unsigned long long down[8] = {};
	HIP_OK(hipMemcpyAsync(down, c.stat, 64, hipMemcpyDeviceToHost, st));
	HIP_OK(hipStreamSynchronize(st));
	if (down[3] >= (1ull << 31)) throw Error(HRY_E_UNSUPPORTED, "intersections: 2^31 pairs or more");
	const uint32_t P = (uint32_t)down[3];

	// ---- ... and of the second behind it: the sort's two sides.  Where the buffer has to grow, the first stretch's pieces move along
	// (without a pair nothing is sorted, and the buffer stays as it is)
	if (P) {
		W.take(c.key, (size_t)P * 4); W.take(c.val, (size_t)P * 4); W.take(key_b, (size_t)P * 4); W.take(val_b, (size_t)P * 4);
		W.take(radix, bvh_pairs_radix_words(P) * 4);
		grow_keeping(cx.d_bvh, W.total, first, st);
		W.bind(cx.d_bvh.p);
		c.words = (uint32_t*)(c.stat + 4);
	}

	// ---- the outputs, in one allocation
	OutputPlan plan;
	plan.add("pairs", P, 2, HRY_UINT);
	plan.add("pair_shared", P, 1, HRY_UINT);
	plan.add("tri_pairs", T, 1, HRY_UINT);
	plan.alloc(cx.device, out);
	c.fill = 1; c.P = P; c.tri_pairs = out.ptr<uint32_t>("tri_pairs");
	if (T) HIP_OK(hipMemsetAsync(c.tri_pairs, 0, (size_t)T * 4, st));

	timer.mark(st);
	launch_bvh_pairs_fill(st, v, c, key_b, val_b, radix, out.ptr<uint32_t>("pairs"), out.ptr<uint32_t>("pair_shared"));
	timer.mark(st);
	uint32_t words[2] = {};
	HIP_OK(hipMemcpyAsync(words, c.words, 8, hipMemcpyDeviceToHost, st));
	HIP_OK(hipStreamSynchronize(st));
	if (words[0] != P) throw Error(HRY_E_INTERNAL, "intersections: the scan of the counts and their sum disagree");
	out.device_ms = timer.ms();
	out.uploaded_bytes = 0;
	out.summary[0] = T; out.summary[1] = down[0]; out.summary[2] = down[1]; out.summary[3] = P; out.summary[4] = words[1]; out.summary[5] = down[2];
}

}   // namespace hry
