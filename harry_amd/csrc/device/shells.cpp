// The shells of a render build's triangles -- components, per-shell counts, boundary loops and, where asked for, area, signed volume
// and box -- built where the render and edges builds lie in HBM (include/harry_amd.h: hry_shells_build; kernels: shells.hip, dedup.hip
// with ShellVertexKey, measures.hip; DESIGN.md "Shells").  Nothing is uploaded; four bytes come down in the middle (S, before the
// outputs are allocated) and twenty at the end (the summary).  The decode's token and the encoder's resident mesh are left alone.
#include <hip/hip_runtime.h>

#include "result_build.hpp"

namespace hry {

using namespace dev;

void shells_build(Context &cx, const Mesh &m, const RenderResult &r, const EdgesResult &e, uint32_t flags, ShellsResult &out)
{
	if (flags & ~(uint32_t)HRY_SHELLS_GEOMETRY) throw Error(HRY_E_ARG, "unknown shells flag");
	const bool geometry = flags & HRY_SHELLS_GEOMETRY;
	const EdgesFit fit = require_edges_of(cx, m, r, e);
	ShellsView v{ tri_adjacency_of(r, fit, m) };   // (what it writes: once the outputs are allocated)
	const uint32_t T = v.ntri, n = v.n, ne = v.ne, nf = v.nf;
	MeasuresView g{};
	if (geometry) g.pos = render_positions(m, r, "shells", g.pos_stride);
	HIP_OK(hipSetDevice(cx.device));

	// ---- the working buffer
	Carve W;
	DedupPlan D;
	D.reserve(W, n, true);   // the corners by (shell, decoded vertex)
	ShellsWork w{};
	W.take(w.par, (size_t)T * 4); W.take(w.flag, (size_t)T * 4); W.take(w.num, ((size_t)T + 1) * 4); W.take(w.sums, scan_sums_words(T) * 4);
	W.take(w.slot, (size_t)n * 4); W.take(w.loop_par, (size_t)ne * 4); W.take(w.summary, 32);
	const size_t w_measures = geometry ? measures_reserve(W, T) : 0;
	cx.d_shells.ensure(W.total);
	void *wb = cx.d_shells.p;
	W.bind(wb);
	D.bind(W, wb);
	w.pair_id = D.ids; w.pair_first_of = D.first_of;
	const MeasuresWork mw = geometry ? measures_bind(W, wb, w_measures, w.flag, w.sums) : MeasuresWork{};
	hipStream_t st = cx.stream;
	StretchTimer timer;

	timer.mark(st);
	launch_shells_roots(st, v, w);
	timer.mark(st);
	uint32_t ns = 0;
	if (T) HIP_OK(hipMemcpyAsync(&ns, w.num + T, 4, hipMemcpyDeviceToHost, st));
	HIP_OK(hipStreamSynchronize(st));
	if (ns > T || (T && !ns)) throw Error(HRY_E_INTERNAL, "shells: the numbering does not fit the triangles");

	// ---- the outputs, in one allocation
	OutputPlan plan;
	plan.add("tri_shell", T, 1, HRY_UINT);
	plan.add("face_shell", T ? nf : 0, 1, HRY_UINT);
	plan.add("edge_shell", ne, 1, HRY_UINT);
	plan.add("shell_first", ns, 1, HRY_UINT);
	plan.add("shell_counts", ns, 8, HRY_UINT);
	if (geometry) plan.add("shell_measures", ns, 8, HRY_FLOAT);
	plan.alloc(cx.device, out);
	auto dst = [&](const char *name) { return out.ptr<uint32_t>(name); };
	v.tri_shell = dst("tri_shell"); v.face_shell = dst("face_shell"); v.edge_shell = dst("edge_shell"); v.first = dst("shell_first"); v.counts = dst("shell_counts");
	v.ns = ns;
	if (geometry) {   // the shells as the labels of the measures
		g.indices = v.indices; g.label = v.tri_shell; g.first = v.first; g.measures = out.ptr<float>("shell_measures");
		g.ntri = T; g.nout = v.nout; g.nl = ns;
	}

	// (the fills lie outside the events, as in render.cpp)
	if (T) {
		HIP_OK(hipMemsetAsync(D.table, 0xff, D.table_bytes(), st));
		HIP_OK(hipMemsetAsync(w.slot, 0xff, (size_t)n * 4, st));
		HIP_OK(hipMemsetAsync(v.face_shell, 0xff, (size_t)nf * 4, st));   // (a face without a triangle: HRY_NO_ELEMENT)
		HIP_OK(hipMemsetAsync(v.counts, 0, (size_t)ns * 32, st));
		if (geometry) measures_clear(st, mw, ns);
	}
	HIP_OK(hipMemsetAsync(w.summary, 0, 32, st));
	timer.mark(st);
	launch_shells_label(st, v, w);
	if (T) {
		ShellVertexView u{};
		u.indices = v.indices; u.vsrc = v.vsrc; u.tri_shell = v.tri_shell; u.nout = v.nout;
		launch_dedup_count(st, u, D);
		launch_dedup_assign(st, D, 0, nullptr);
	}
	launch_shells_counts(st, v, w);
	if (geometry) launch_measures(st, g, mw);
	timer.mark(st);
	uint32_t sum[5] = {};
	HIP_OK(hipMemcpyAsync(sum, w.summary, sizeof sum, hipMemcpyDeviceToHost, st));
	HIP_OK(hipStreamSynchronize(st));
	out.device_ms = timer.ms();
	out.uploaded_bytes = 0;
	out.summary[0] = ns;
	for (int i = 0; i < 5; ++i) out.summary[1 + i] = sum[i];
}

}   // namespace hry
