// A consistent winding of a render build's triangles, patch by patch -- which triangles to turn, which patches cannot be oriented,
// and, where asked for, which way is outward -- built where the render and edges builds lie in HBM (include/harry_amd.h:
// hry_orient_build; kernels: orient.hip, and the measures of shells.hip over the patches; DESIGN.md "Orientation").  Nothing is
// uploaded; four bytes come down in the middle (P, before the outputs are allocated) and twenty at the end (the summary).  The
// decode's token and the encoder's resident mesh are left alone.
#include <hip/hip_runtime.h>

#include "context.hpp"
#include "kernels.hpp"

namespace hry {

using namespace dev;

void orient_build(Context &cx, const Mesh &m, const RenderResult &r, const EdgesResult &e, uint32_t flags, OrientResult &out)
{
	if (flags & ~(uint32_t)(HRY_ORIENT_MAJORITY | HRY_ORIENT_OUTWARD)) throw Error(HRY_E_ARG, "unknown orient flag");
	const bool majority = flags & HRY_ORIENT_MAJORITY, outward = flags & HRY_ORIENT_OUTWARD;
	const EdgesFit fit = require_edges_of(cx, m, r, e);
	const uint64_t ntri = m.ntri();
	const uint32_t T = (uint32_t)ntri, n = (uint32_t)(3 * ntri), nf = (uint32_t)m.nf;
	uint32_t pos_stride = 0;
	const float *pos = outward ? render_positions(m, r, "orient", pos_stride) : nullptr;
	HIP_OK(hipSetDevice(cx.device));

	// ---- the working buffer
	Carve W;
	const size_t w_par = W.reserve((size_t)T * 8), w_flag = W.reserve((size_t)T * 4), w_num = W.reserve(((size_t)T + 1) * 4), w_sums = W.reserve(scan_sums_words(T) * 4);
	const size_t w_turn = W.reserve((size_t)T * 4), w_summary = W.reserve(32);
	size_t w_partial = 0, w_pcount = 0, w_pstart = 0, w_pseg = 0, w_lo = 0, w_hi = 0, w_hubs = 0;
	if (outward) {   // (P <= T of everything per patch)
		w_partial = W.reserve((size_t)T * 16); w_pcount = W.reserve((size_t)T * 4); w_pstart = W.reserve(((size_t)T + 1) * 4); w_pseg = W.reserve((size_t)T * 4);
		w_lo = W.reserve((size_t)T * 12); w_hi = W.reserve((size_t)T * 12); w_hubs = W.reserve(((size_t)shells_hub_capacity(T) + 1) * 4);
	}
	cx.d_orient.ensure(W.total);
	void *wb = cx.d_orient.p;
	OrientWork w{};
	w.par = W.ptr<uint32_t>(wb, w_par); w.flag = W.ptr<uint32_t>(wb, w_flag); w.num = W.ptr<uint32_t>(wb, w_num); w.sums = W.ptr<uint32_t>(wb, w_sums);
	w.turn = W.ptr<uint32_t>(wb, w_turn); w.summary = W.ptr<uint32_t>(wb, w_summary);
	ShellsWork sw{};   // the measures' share (shells.hip)
	sw.flag = w.flag; sw.sums = w.sums;
	if (outward) {
		sw.partial = W.ptr<double>(wb, w_partial); sw.pcount = W.ptr<uint32_t>(wb, w_pcount); sw.pstart = W.ptr<uint32_t>(wb, w_pstart); sw.pseg = W.ptr<uint32_t>(wb, w_pseg);
		sw.box_lo = W.ptr<uint32_t>(wb, w_lo); sw.box_hi = W.ptr<uint32_t>(wb, w_hi); sw.hubs = W.ptr<uint32_t>(wb, w_hubs);
	}
	hipStream_t st = cx.stream;
	TimedEvent ev[4];

	OrientView v{};
	v.indices = (const uint32_t*)r.find("indices")->p; v.vsrc = (const uint32_t*)r.find("vertex_source")->p; v.tri_face = (const uint32_t*)r.find("tri_face")->p;
	v.tri_edges = (const uint32_t*)fit.tri_edges->p; v.offsets = (const uint32_t*)fit.offsets->p; v.sides = (const uint32_t*)fit.sides->p;
	v.n = n; v.ntri = T; v.nout = r.nverts; v.nf = nf; v.ne = fit.ne;
	HIP_OK(hipEventRecord(ev[0], st));
	launch_orient_roots(st, v, w);
	HIP_OK(hipEventRecord(ev[1], st));
	uint32_t np = 0;
	if (T) HIP_OK(hipMemcpyAsync(&np, w.num + T, 4, hipMemcpyDeviceToHost, st));
	HIP_OK(hipStreamSynchronize(st));
	if (np > T || (T && !np)) throw Error(HRY_E_INTERNAL, "orient: the numbering does not fit the triangles");

	// ---- the outputs, in one allocation
	Carve O;
	struct Plan { const char *name; uint64_t rows; int width, type; size_t slot; };
	std::vector<Plan> plan;
	auto add = [&](const char *name, uint64_t rows, int width, int type) { plan.push_back(Plan{ name, rows, width, type, O.reserve((size_t)rows * width * 4) }); };
	add("tri_patch", T, 1, HRY_UINT);
	add("tri_flip", T, 1, HRY_UINT);
	add("face_flip", T ? nf : 0, 1, HRY_UINT);
	add("oriented_indices", T, 3, HRY_UINT);
	add("patch_first", np, 1, HRY_UINT);
	add("patch_counts", np, 8, HRY_UINT);
	if (outward) add("patch_measures", np, 8, HRY_FLOAT);
	out.block.alloc(cx.device, O.total);
	for (const Plan &p : plan) out.bufs.push_back(NamedBuf{ p.name, O.ptr<void>(out.block.p, p.slot), p.rows, p.width, p.type });
	auto dst = [&](const char *name) { return (uint32_t*)out.find(name)->p; };
	v.tri_patch = dst("tri_patch"); v.tri_flip = dst("tri_flip"); v.face_flip = dst("face_flip"); v.oriented = dst("oriented_indices");
	v.first = dst("patch_first"); v.counts = dst("patch_counts");
	v.np = np;
	if (outward) v.measures = (float*)dst("patch_measures");

	// (the fills lie outside the events, as in render.cpp)
	if (T) {
		HIP_OK(hipMemsetAsync(v.face_flip, 0, (size_t)nf * 4, st));   // (a face without a triangle: 0)
		HIP_OK(hipMemsetAsync(v.counts, 0, (size_t)np * 32, st));
		HIP_OK(hipMemsetAsync(w.turn, 0, (size_t)np * 4, st));
		if (outward) {
			HIP_OK(hipMemsetAsync(sw.pcount, 0, (size_t)np * 4, st));
			HIP_OK(hipMemsetAsync(sw.box_lo, 0xff, (size_t)np * 12, st));
			HIP_OK(hipMemsetAsync(sw.box_hi, 0, (size_t)np * 12, st));
			HIP_OK(hipMemsetAsync(sw.hubs, 0, 4, st));
		}
	}
	HIP_OK(hipMemsetAsync(w.summary, 0, 32, st));
	HIP_OK(hipEventRecord(ev[2], st));
	launch_orient_flips(st, v, w, majority);
	if (outward) {
		// the patches as the shells of the measures: their labels, their lowest triangles, the triangles as oriented so far
		ShellsView sv{};
		sv.indices = v.oriented; sv.vsrc = v.vsrc; sv.tri_face = v.tri_face; sv.tri_edges = v.tri_edges; sv.offsets = v.offsets; sv.sides = v.sides;
		sv.tri_shell = v.tri_patch; sv.first = v.first; sv.counts = v.counts;
		sv.pos = pos; sv.pos_stride = pos_stride; sv.measures = v.measures;
		sv.n = n; sv.ntri = T; sv.nout = r.nverts; sv.nf = nf; sv.ne = fit.ne; sv.ns = np;
		launch_shells_measures(st, sv, sw);
		launch_orient_outward(st, v, w);
	}
	launch_orient_summary(st, v, w);
	HIP_OK(hipEventRecord(ev[3], st));
	uint32_t sum[5] = {};
	HIP_OK(hipMemcpyAsync(sum, w.summary, sizeof sum, hipMemcpyDeviceToHost, st));
	HIP_OK(hipStreamSynchronize(st));
	float a = 0, c = 0;
	HIP_OK(hipEventElapsedTime(&a, ev[0], ev[1]));
	HIP_OK(hipEventElapsedTime(&c, ev[2], ev[3]));
	out.device_ms = (double)a + (double)c;
	out.uploaded_bytes = 0;
	out.summary[0] = np;
	for (int i = 0; i < 5; ++i) out.summary[1 + i] = sum[i];
}

}   // namespace hry
