// The hierarchy over the triangles of a render build, built where the render build lies in HBM, and the ray cast over it
// (include/harry_amd.h: hry_bvh_build, hry_bvh_cast; kernels: bvh.hip; DESIGN.md "Bvh").  The build uploads nothing: it reads the
// render result's indices and the float rows of its position list; sixty-four bytes come down between its two stretches (the number
// of leaves sizes the buffers, the depth counts the launches of the box fit).  The result keeps its own copy of the leaves'
// positions, so the render build may be freed.  The decode's token and the encoder's resident mesh are left alone.
#include <hip/hip_runtime.h>

#include <cmath>

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
void check_host_memory(const void *p, const char *what)
{
	hipPointerAttribute_t a{};
	const hipError_t e = hipPointerGetAttributes(&a, p);
	if (e != hipSuccess) { (void)hipGetLastError(); return; }
	if (a.type == hipMemoryTypeDevice) throw Error(HRY_E_ARG, std::string(what) + ": device memory in a cast with HRY_CAST_HOST");
}

}   // namespace

void bvh_cast(Context &cx, const BvhResult &b, uint64_t n, const float *origins, uint64_t origin_stride, const float *dirs, uint64_t dir_stride, double tmin, double tmax,
              uint32_t flags, uint32_t *hit_tri, float *hit_t, float *hit_uv, uint64_t *stat, double *device_ms)
{
	if (flags & ~(uint32_t)HRY_CAST_HOST) throw Error(HRY_E_ARG, "unknown cast flag");
	if (origin_stride % 4 || dir_stride % 4) throw Error(HRY_E_ARG, "cast: a stride is not a multiple of 4");
	if (std::isnan(tmin) || std::isnan(tmax)) throw Error(HRY_E_ARG, "cast: tmin or tmax is NaN");
	if (b.block.device != cx.device) throw Error(HRY_E_ARG, "the hierarchy lives on another device than the context's");
	if (stat) stat[0] = stat[1] = 0;
	if (device_ms) *device_ms = 0.0;
	if (!n) return;
	if (n > (1ull << 40) / std::max<uint64_t>(std::max(origin_stride, dir_stride), 12)) throw Error(HRY_E_UNSUPPORTED, "cast: more than 2^40 bytes of rays");
	const bool host = (flags & HRY_CAST_HOST) != 0;
	const uint64_t o_bytes = (n - 1) * origin_stride + 12, d_bytes = (n - 1) * dir_stride + 12;
	if (((uintptr_t)origins | (uintptr_t)dirs | (uintptr_t)hit_tri | (uintptr_t)hit_t | (uintptr_t)hit_uv) % 4) throw Error(HRY_E_ARG, "cast: a misaligned pointer");
	HIP_OK(hipSetDevice(cx.device));
	if (host) {
		check_host_memory(origins, "origins"); check_host_memory(dirs, "dirs"); check_host_memory(hit_tri, "hit_tri");
		if (hit_t) check_host_memory(hit_t, "hit_t");
		if (hit_uv) check_host_memory(hit_uv, "hit_uv");
	} else {
		check_device_memory(cx, origins, o_bytes, "origins"); check_device_memory(cx, dirs, d_bytes, "dirs"); check_device_memory(cx, hit_tri, n * 4, "hit_tri");
		if (hit_t) check_device_memory(cx, hit_t, n * 4, "hit_t");
		if (hit_uv) check_device_memory(cx, hit_uv, n * 8, "hit_uv");
	}

	// ---- the working buffer: the two counters; with HRY_CAST_HOST the staged rays and results behind them
	Carve W;
	BvhCast c{};
	c.n = n; c.o_stride = origin_stride; c.d_stride = dir_stride; c.tmin = tmin; c.tmax = tmax;
	uint8_t *s_o, *s_d;
	uint32_t *s_tri;
	float *s_t, *s_uv;
	W.take(c.stat, 16); W.take(s_o, host ? o_bytes : 0); W.take(s_d, host ? d_bytes : 0); W.take(s_tri, host ? n * 4 : 0);
	W.take(s_t, host && hit_t ? n * 4 : 0); W.take(s_uv, host && hit_uv ? n * 8 : 0);
	cx.d_bvh.ensure(W.total);
	W.bind(cx.d_bvh.p);
	hipStream_t st = cx.stream;
	if (host) {
		c.o = s_o; c.d = s_d; c.hit_tri = s_tri; c.hit_t = hit_t ? s_t : nullptr; c.hit_uv = hit_uv ? s_uv : nullptr;
		HIP_OK(hipMemcpyAsync((void*)c.o, origins, o_bytes, hipMemcpyHostToDevice, st));
		HIP_OK(hipMemcpyAsync((void*)c.d, dirs, d_bytes, hipMemcpyHostToDevice, st));
	} else {
		c.o = (const uint8_t*)origins; c.d = (const uint8_t*)dirs; c.hit_tri = hit_tri; c.hit_t = hit_t; c.hit_uv = hit_uv;
	}
	HIP_OK(hipMemsetAsync(c.stat, 0, 16, st));
	StretchTimer timer;
	timer.mark(st);
	launch_bvh_cast(st, bvh_view_of(b), c);
	timer.mark(st);   // (one stretch)
	unsigned long long counters[2] = {};
	HIP_OK(hipMemcpyAsync(counters, c.stat, 16, hipMemcpyDeviceToHost, st));
	if (host) {
		HIP_OK(hipMemcpyAsync(hit_tri, c.hit_tri, n * 4, hipMemcpyDeviceToHost, st));
		if (hit_t) HIP_OK(hipMemcpyAsync(hit_t, c.hit_t, n * 4, hipMemcpyDeviceToHost, st));
		if (hit_uv) HIP_OK(hipMemcpyAsync(hit_uv, c.hit_uv, n * 8, hipMemcpyDeviceToHost, st));
	}
	HIP_OK(hipStreamSynchronize(st));
	if (stat) { stat[0] = counters[0]; stat[1] = counters[1]; }
	if (device_ms) *device_ms = timer.ms();
}

}   // namespace hry
