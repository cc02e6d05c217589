// Vertex areas and curvatures of a render build, built where the render and edges builds lie in HBM (include/harry_amd.h:
// hry_curvature_build; kernels: curvature.hip; DESIGN.md "Curvature").  Nothing is uploaded: the build reads the render result's
// indices, vertex_source and the float rows of its position list, and the edges result's edge_offsets and edge_sides; fifty-six
// bytes come down at the end (the summary's counters and the totals).  The decode's token and the encoder's resident mesh are left
// alone.
#include <hip/hip_runtime.h>

#include "result_build.hpp"

namespace hry {

using namespace dev;

void curvature_build(Context &cx, const Mesh &m, const RenderResult &r, const EdgesResult &e, uint32_t flags, CurvatureResult &out)
{
	if (flags) throw Error(HRY_E_ARG, "unknown curvature flag");
	const EdgesFit fit = require_edges_of(cx, m, r, e);
	CurvView v{ tri_adjacency_of(r, fit, m) };
	const uint32_t n = v.n, nout = v.nout, nv = (uint32_t)m.nv;
	v.pos = render_positions(m, r, "curvature", v.pos_stride);
	v.nv = nv;
	HIP_OK(hipSetDevice(cx.device));

	// ---- the working buffer (CurvWork, dev_types.hpp)
	Carve W;
	const uint32_t fold1 = curvature_fold_rows(nv), fold2 = curvature_fold_rows(fold1);
	CurvWork w{};
	W.take(w.terms, (size_t)nv * 24); W.take(w.fold_a, ((size_t)fold1 + 1) * 24); W.take(w.fold_b, ((size_t)fold2 + 1) * 24);
	W.take(w.ends, (size_t)nv * 4); W.take(w.count, (size_t)nv * 4); W.take(w.start, ((size_t)nv + 1) * 4);
	W.take(w.sums, scan_sums_words(nv) * 4); W.take(w.seg, (size_t)n * 4); W.take(w.hubs, ((size_t)curvature_hub_capacity(n) + 1) * 4);
	W.take(w.cls, (size_t)nv * 4); W.take(w.rows, (size_t)nv * 28); W.take(w.classes, 32);
	cx.d_curvature.ensure(W.total);
	W.bind(cx.d_curvature.p);

	// ---- the outputs, in one allocation
	OutputPlan plan;
	plan.add("vertex_class", nout, 1, HRY_UINT);
	plan.add("vertex_area", nout, 1, HRY_FLOAT);
	plan.add("angle_defect", nout, 1, HRY_FLOAT);
	plan.add("gaussian", nout, 1, HRY_FLOAT);
	plan.add("mean_normal", nout, 3, HRY_FLOAT);
	plan.add("mean", nout, 1, HRY_FLOAT);
	plan.alloc(cx.device, out);
	auto dst = [&](const char *name) { return out.ptr<float>(name); };
	v.vertex_class = out.ptr<uint32_t>("vertex_class"); v.area = dst("vertex_area"); v.defect = dst("angle_defect"); v.gaussian = dst("gaussian");
	v.mean_normal = dst("mean_normal"); v.mean = dst("mean");

	hipStream_t st = cx.stream;
	StretchTimer timer;
	// (the fills lie outside the events, as in render.cpp)
	if (nv) {
		HIP_OK(hipMemsetAsync(w.ends, 0, (size_t)nv * 4, st));
		HIP_OK(hipMemsetAsync(w.count, 0, (size_t)nv * 4, st));
	}
	HIP_OK(hipMemsetAsync(w.hubs, 0, 4, st));
	HIP_OK(hipMemsetAsync(w.classes, 0, 32, st));
	timer.mark(st);
	const double *d_totals = launch_curvature(st, v, w);
	timer.mark(st);   // (one stretch: nothing comes down in between)
	uint32_t cls[8] = {};
	HIP_OK(hipMemcpyAsync(cls, w.classes, 32, hipMemcpyDeviceToHost, st));
	if (d_totals) HIP_OK(hipMemcpyAsync(out.totals, d_totals, 24, hipMemcpyDeviceToHost, st));
	HIP_OK(hipStreamSynchronize(st));
	out.device_ms = timer.ms();
	out.uploaded_bytes = 0;
	out.summary[0] = nv; out.summary[1] = cls[0]; out.summary[2] = cls[1]; out.summary[3] = cls[2]; out.summary[4] = cls[3]; out.summary[5] = cls[4];
}

}   // namespace hry
