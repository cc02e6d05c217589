// The shells of a render build's triangles -- components, per-shell counts, boundary loops and, where asked for, area, signed volume
// and box -- built where the render and edges builds lie in HBM (include/harry_amd.h: hry_shells_build; kernels: shells.hip, dedup.hip
// with ShellVertexKey; DESIGN.md "Shells").  Nothing is uploaded; four bytes come down in the middle (S, before the outputs are
// allocated) and twenty at the end (the summary).  The decode's token and the encoder's resident mesh are left alone.
#include <hip/hip_runtime.h>

#include "context.hpp"
#include "kernels.hpp"

namespace hry {

using namespace dev;

EdgesFit require_edges_of(const Context &cx, const Mesh &m, const RenderResult &r, const EdgesResult &e)
{
	require_render_of(cx, m, r);
	if (e.block.device != cx.device) throw Error(HRY_E_ARG, "the edge buffers live on another device than the context's");
	const uint64_t ntri = m.ntri(), ne64 = e.summary[0];
	const uint32_t n = (uint32_t)(3 * ntri);
	// ---- is e an edges build of (m, r)?
	const NamedBuf *b_te = e.find("tri_edges"), *b_ed = e.find("edges"), *b_off = e.find("edge_offsets"), *b_sides = e.find("edge_sides");
	const bool fits = b_te && b_ed && b_off && b_sides && b_te->rows == ntri && b_te->width == 3 && b_ed->rows == ne64 && b_off->rows == ne64 + 1 &&
	                  b_sides->rows == n && ne64 <= n && (n == 0) == (ne64 == 0);
	if (!fits) throw Error(HRY_E_ARG, "the edge buffers are not an edges build of this mesh's render build (triangles or edges differ)");
	return EdgesFit{ b_te, b_off, b_sides, (uint32_t)ne64 };
}

void shells_build(Context &cx, const Mesh &m, const RenderResult &r, const EdgesResult &e, uint32_t flags, ShellsResult &out)
{
	if (flags & ~(uint32_t)HRY_SHELLS_GEOMETRY) throw Error(HRY_E_ARG, "unknown shells flag");
	const bool geometry = flags & HRY_SHELLS_GEOMETRY;
	const EdgesFit fit = require_edges_of(cx, m, r, e);
	const NamedBuf *b_te = fit.tri_edges, *b_off = fit.offsets, *b_sides = fit.sides;
	const uint64_t ntri = m.ntri();
	const uint32_t n = (uint32_t)(3 * ntri), ne = fit.ne, nf = (uint32_t)m.nf;
	uint32_t pos_stride = 0;
	const float *pos = geometry ? render_positions(m, r, "shells", pos_stride) : nullptr;
	HIP_OK(hipSetDevice(cx.device));

	// ---- the working buffer
	const uint32_t T = (uint32_t)ntri;
	Carve W;
	DedupPlan D;
	D.reserve(W, n, true);   // the corners by (shell, decoded vertex)
	const size_t w_par = W.reserve((size_t)T * 4), w_flag = W.reserve((size_t)T * 4), w_num = W.reserve(((size_t)T + 1) * 4), w_sums = W.reserve(scan_sums_words(T) * 4);
	const size_t w_slot = W.reserve((size_t)n * 4), w_loop = W.reserve((size_t)ne * 4), w_summary = W.reserve(32);
	size_t w_partial = 0, w_pcount = 0, w_pstart = 0, w_pseg = 0, w_lo = 0, w_hi = 0, w_hubs = 0;
	if (geometry) {   // (S <= T of everything per shell)
		w_partial = W.reserve((size_t)T * 16); w_pcount = W.reserve((size_t)T * 4); w_pstart = W.reserve(((size_t)T + 1) * 4); w_pseg = W.reserve((size_t)T * 4);
		w_lo = W.reserve((size_t)T * 12); w_hi = W.reserve((size_t)T * 12); w_hubs = W.reserve(((size_t)shells_hub_capacity(T) + 1) * 4);
	}
	cx.d_shells.ensure(W.total);
	void *wb = cx.d_shells.p;
	D.bind(W, wb);
	ShellsWork w{};
	w.par = W.ptr<uint32_t>(wb, w_par); w.flag = W.ptr<uint32_t>(wb, w_flag); w.num = W.ptr<uint32_t>(wb, w_num); w.sums = W.ptr<uint32_t>(wb, w_sums);
	w.pair_id = D.ids; w.pair_first_of = D.first_of; w.slot = W.ptr<uint32_t>(wb, w_slot); w.loop_par = W.ptr<uint32_t>(wb, w_loop);
	w.summary = W.ptr<uint32_t>(wb, w_summary);
	if (geometry) {
		w.partial = W.ptr<double>(wb, w_partial); w.pcount = W.ptr<uint32_t>(wb, w_pcount); w.pstart = W.ptr<uint32_t>(wb, w_pstart); w.pseg = W.ptr<uint32_t>(wb, w_pseg);
		w.box_lo = W.ptr<uint32_t>(wb, w_lo); w.box_hi = W.ptr<uint32_t>(wb, w_hi); w.hubs = W.ptr<uint32_t>(wb, w_hubs);
	}
	hipStream_t st = cx.stream;
	TimedEvent ev[4];

	ShellsView v{};
	v.indices = (const uint32_t*)r.find("indices")->p; v.vsrc = (const uint32_t*)r.find("vertex_source")->p; v.tri_face = (const uint32_t*)r.find("tri_face")->p;
	v.tri_edges = (const uint32_t*)b_te->p; v.offsets = (const uint32_t*)b_off->p; v.sides = (const uint32_t*)b_sides->p;
	v.n = n; v.ntri = T; v.nout = r.nverts; v.nf = nf; v.ne = ne;
	HIP_OK(hipEventRecord(ev[0], st));
	launch_shells_roots(st, v, w);
	HIP_OK(hipEventRecord(ev[1], st));
	uint32_t ns = 0;
	if (T) HIP_OK(hipMemcpyAsync(&ns, w.num + T, 4, hipMemcpyDeviceToHost, st));
	HIP_OK(hipStreamSynchronize(st));
	if (ns > T || (T && !ns)) throw Error(HRY_E_INTERNAL, "shells: the numbering does not fit the triangles");

	// ---- the outputs, in one allocation
	Carve O;
	struct Plan { const char *name; uint64_t rows; int width, type; size_t slot; };
	std::vector<Plan> plan;
	auto add = [&](const char *name, uint64_t rows, int width, int type) { plan.push_back(Plan{ name, rows, width, type, O.reserve((size_t)rows * width * 4) }); };
	add("tri_shell", T, 1, HRY_UINT);
	add("face_shell", T ? nf : 0, 1, HRY_UINT);
	add("edge_shell", ne, 1, HRY_UINT);
	add("shell_first", ns, 1, HRY_UINT);
	add("shell_counts", ns, 8, HRY_UINT);
	if (geometry) add("shell_measures", ns, 8, HRY_FLOAT);
	out.block.alloc(cx.device, O.total);
	for (const Plan &p : plan) out.bufs.push_back(NamedBuf{ p.name, O.ptr<void>(out.block.p, p.slot), p.rows, p.width, p.type });
	auto dst = [&](const char *name) { return (uint32_t*)out.find(name)->p; };
	v.tri_shell = dst("tri_shell"); v.face_shell = dst("face_shell"); v.edge_shell = dst("edge_shell"); v.first = dst("shell_first"); v.counts = dst("shell_counts");
	v.ns = ns;
	if (geometry) { v.pos = pos; v.pos_stride = pos_stride; v.measures = (float*)dst("shell_measures"); }

	// (the fills lie outside the events, as in render.cpp)
	if (T) {
		HIP_OK(hipMemsetAsync(D.table, 0xff, D.table_bytes(), st));
		HIP_OK(hipMemsetAsync(w.slot, 0xff, (size_t)n * 4, st));
		HIP_OK(hipMemsetAsync(v.face_shell, 0xff, (size_t)nf * 4, st));   // (a face without a triangle: HRY_NO_ELEMENT)
		HIP_OK(hipMemsetAsync(v.counts, 0, (size_t)ns * 32, st));
		if (geometry) {
			HIP_OK(hipMemsetAsync(w.pcount, 0, (size_t)ns * 4, st));
			HIP_OK(hipMemsetAsync(w.box_lo, 0xff, (size_t)ns * 12, st));
			HIP_OK(hipMemsetAsync(w.box_hi, 0, (size_t)ns * 12, st));
			HIP_OK(hipMemsetAsync(w.hubs, 0, 4, st));
		}
	}
	HIP_OK(hipMemsetAsync(w.summary, 0, 32, st));
	HIP_OK(hipEventRecord(ev[2], st));
	launch_shells_label(st, v, w);
	if (T) {
		ShellVertexView u{};
		u.indices = v.indices; u.vsrc = v.vsrc; u.tri_shell = v.tri_shell; u.nout = v.nout;
		launch_dedup_count(st, u, D);
		launch_dedup_assign(st, D, 0, nullptr);
	}
	launch_shells_counts(st, v, w);
	launch_shells_measures(st, v, w);
	HIP_OK(hipEventRecord(ev[3], st));
	uint32_t sum[5] = {};
	HIP_OK(hipMemcpyAsync(sum, w.summary, sizeof sum, hipMemcpyDeviceToHost, st));
	HIP_OK(hipStreamSynchronize(st));
	float a = 0, c = 0;
	HIP_OK(hipEventElapsedTime(&a, ev[0], ev[1]));
	HIP_OK(hipEventElapsedTime(&c, ev[2], ev[3]));
	out.device_ms = (double)a + (double)c;
	out.uploaded_bytes = 0;
	out.summary[0] = ns;
	for (int i = 0; i < 5; ++i) out.summary[1 + i] = sum[i];
}

}   // namespace hry
