// A consistent winding of a render build's triangles, patch by patch -- which triangles to turn, which patches cannot be oriented,
// and, where asked for, which way is outward -- built where the render and edges builds lie in HBM (include/harry_amd.h:
// hry_orient_build; kernels: orient.hip, and measures.hip over the patches; DESIGN.md "Orientation").  Nothing is uploaded; four
// bytes come down in the middle (P, before the outputs are allocated) and twenty at the end (the summary).  The decode's token and
// the encoder's resident mesh are left alone.
#include <hip/hip_runtime.h>

#include "result_build.hpp"

namespace hry {

using namespace dev;

void orient_build(Context &cx, const Mesh &m, const RenderResult &r, const EdgesResult &e, uint32_t flags, OrientResult &out)
{
	if (flags & ~(uint32_t)(HRY_ORIENT_MAJORITY | HRY_ORIENT_OUTWARD)) throw Error(HRY_E_ARG, "unknown orient flag");
	const bool majority = flags & HRY_ORIENT_MAJORITY, outward = flags & HRY_ORIENT_OUTWARD;
	const EdgesFit fit = require_edges_of(cx, m, r, e);
	OrientView v{ tri_adjacency_of(r, fit, m) };   // (what it writes: once the outputs are allocated)
	const uint32_t T = v.ntri, nf = v.nf;
	MeasuresView g{};
	if (outward) g.pos = render_positions(m, r, "orient", g.pos_stride);
	HIP_OK(hipSetDevice(cx.device));

	// ---- the working buffer
	Carve W;
	OrientWork w{};
	W.take(w.par, (size_t)T * 8); W.take(w.flag, (size_t)T * 4); W.take(w.num, ((size_t)T + 1) * 4); W.take(w.sums, scan_sums_words(T) * 4);
	W.take(w.turn, (size_t)T * 4); W.take(w.summary, 32);
	const size_t w_measures = outward ? measures_reserve(W, T) : 0;
	cx.d_orient.ensure(W.total);
	void *wb = cx.d_orient.p;
	W.bind(wb);
	const MeasuresWork mw = outward ? measures_bind(W, wb, w_measures, w.flag, w.sums) : MeasuresWork{};
	hipStream_t st = cx.stream;
	StretchTimer timer;

	timer.mark(st);
	launch_orient_roots(st, v, w);
	timer.mark(st);
	uint32_t np = 0;
	if (T) HIP_OK(hipMemcpyAsync(&np, w.num + T, 4, hipMemcpyDeviceToHost, st));
	HIP_OK(hipStreamSynchronize(st));
	if (np > T || (T && !np)) throw Error(HRY_E_INTERNAL, "orient: the numbering does not fit the triangles");

	// ---- the outputs, in one allocation
	OutputPlan plan;
	plan.add("tri_patch", T, 1, HRY_UINT);
	plan.add("tri_flip", T, 1, HRY_UINT);
	plan.add("face_flip", T ? nf : 0, 1, HRY_UINT);
	plan.add("oriented_indices", T, 3, HRY_UINT);
	plan.add("patch_first", np, 1, HRY_UINT);
	plan.add("patch_counts", np, 8, HRY_UINT);
	if (outward) plan.add("patch_measures", np, 8, HRY_FLOAT);
	plan.alloc(cx.device, out);
	auto dst = [&](const char *name) { return out.ptr<uint32_t>(name); };
	v.tri_patch = dst("tri_patch"); v.tri_flip = dst("tri_flip"); v.face_flip = dst("face_flip"); v.oriented = dst("oriented_indices");
	v.first = dst("patch_first"); v.counts = dst("patch_counts");
	v.np = np;
	if (outward) {   // the patches as the labels of the measures, over the triangles as oriented so far
		v.measures = out.ptr<float>("patch_measures");
		g.indices = v.oriented; g.label = v.tri_patch; g.first = v.first; g.measures = v.measures;
		g.ntri = T; g.nout = v.nout; g.nl = np;
	}

	// (the fills lie outside the events, as in render.cpp)
	if (T) {
		HIP_OK(hipMemsetAsync(v.face_flip, 0, (size_t)nf * 4, st));   // (a face without a triangle: 0)
		HIP_OK(hipMemsetAsync(v.counts, 0, (size_t)np * 32, st));
		HIP_OK(hipMemsetAsync(w.turn, 0, (size_t)np * 4, st));
		if (outward) measures_clear(st, mw, np);
	}
	HIP_OK(hipMemsetAsync(w.summary, 0, 32, st));
	timer.mark(st);
	launch_orient_flips(st, v, w, majority);
	if (outward) {
		launch_measures(st, g, mw);
		launch_orient_outward(st, v, w);
	}
	launch_orient_summary(st, v, w);
	timer.mark(st);
	uint32_t sum[5] = {};
	HIP_OK(hipMemcpyAsync(sum, w.summary, sizeof sum, hipMemcpyDeviceToHost, st));
	HIP_OK(hipStreamSynchronize(st));
	out.device_ms = timer.ms();
	out.uploaded_bytes = 0;
	out.summary[0] = np;
	for (int i = 0; i < 5; ++i) out.summary[1 + i] = sum[i];
}

}   // namespace hry
