// Hard edges and split normals of a render build, built where the render and edges builds lie in HBM (include/harry_amd.h:
// hry_creases_build; kernels: creases.hip, dedup.hip with CreaseKey; DESIGN.md "Creases").  Nothing is uploaded: the build reads the
// render result's indices, vertex_source, tri_face and the float rows of its position list, and the edges result's edge_offsets,
// edge_sides and edge_cos; eight bytes come down in the middle (W and G, before the outputs are allocated) and sixteen at the end (the
// summary's counters).  The decode's token and the encoder's resident mesh are left alone.
#include <hip/hip_runtime.h>

#include <cmath>

#include "result_build.hpp"

namespace hry {

using namespace dev;

void creases_build(Context &cx, const Mesh &m, const RenderResult &r, const EdgesResult &e, double cos_limit, uint32_t flags, CreasesResult &out)
{
	if (flags & ~(uint32_t)HRY_CREASES_ANGLE_WEIGHTED) throw Error(HRY_E_ARG, "unknown creases flag");
	if (std::isnan(cos_limit)) throw Error(HRY_E_ARG, "creases: the limit is not a number");
	const EdgesFit fit = require_edges_of(cx, m, r, e);
	CreaseView v{ tri_adjacency_of(r, fit, m) };   // (what it writes: once the outputs are allocated)
	const uint32_t T = v.ntri, n = v.n, ne = v.ne;
	const NamedBuf *b_cos = e.find("edge_cos");
	if (!b_cos) throw Error(HRY_E_ARG, "creases: the edges build has no \"edge_cos\" (build it with HRY_EDGES_GEOMETRY)");
	if (b_cos->rows != ne || b_cos->width != 1 || b_cos->type != HRY_FLOAT) throw Error(HRY_E_ARG, "the edge buffers do not hold this mesh's edge_cos");
	v.edge_cos = (const float*)b_cos->p;
	v.pos = render_positions(m, r, "creases", v.pos_stride);
	v.cos_limit = cos_limit; v.angle = (flags & HRY_CREASES_ANGLE_WEIGHTED) ? 1 : 0; v.nv = (uint32_t)m.nv;
	HIP_OK(hipSetDevice(cx.device));

	// ---- the working buffer (CreaseWork, dev_types.hpp): count lies where flag lay and seg where par lay, both free by then
	Carve W;
	DedupPlan D;
	D.reserve(W, n, false);   // (the ids are the output buffer indices)
	CreaseWork w{};
	W.take(w.par, (size_t)n * 4); W.take(w.root, (size_t)n * 4); W.take(w.flag, (size_t)n * 4); W.take(w.num, ((size_t)n + 1) * 4);
	W.take(w.sums, scan_sums_words(n) * 4); W.take(w.eclass, (size_t)ne * 4); W.take(w.first_slot, (size_t)n * 4); W.take(w.terms, (size_t)T * 24);
	W.take(w.start, ((size_t)n + 1) * 4); W.take(w.gnormal, (size_t)n * 12); W.take(w.vgroups, (size_t)v.nv * 4);
	W.take(w.hubs, ((size_t)creases_hub_capacity(n) + 1) * 4); W.take(w.classes, 16);
	cx.d_creases.ensure(W.total);
	W.bind(cx.d_creases.p);
	D.bind(W, cx.d_creases.p);
	w.count = w.flag; w.seg = w.par;
	hipStream_t st = cx.stream;
	StretchTimer timer;

	// (the fills lie outside the events, as in render.cpp)
	if (n) HIP_OK(hipMemsetAsync(D.table, 0xff, D.table_bytes(), st));
	HIP_OK(hipMemsetAsync(w.classes, 0, 16, st));
	timer.mark(st);
	launch_creases_groups(st, v, w);
	if (n) {
		CreaseSlotView u{};
		u.indices = v.indices; u.root = w.root;
		launch_dedup_count(st, u, D);
	}
	timer.mark(st);
	uint32_t nw = 0, ng = 0;
	if (n) {
		HIP_OK(hipMemcpyAsync(&nw, D.total(), 4, hipMemcpyDeviceToHost, st));
		HIP_OK(hipMemcpyAsync(&ng, w.num + n, 4, hipMemcpyDeviceToHost, st));
	}
	HIP_OK(hipStreamSynchronize(st));
	if (nw > n || ng > nw || (n && !ng)) throw Error(HRY_E_INTERNAL, "creases: the numberings do not fit the slots");

	// ---- the outputs, in one allocation
	OutputPlan plan;
	plan.add("indices", T, 3, HRY_UINT);
	plan.add("render_vertex", nw, 1, HRY_UINT);
	plan.add("vertex_source", nw, 1, HRY_UINT);
	plan.add("normals", nw, 3, HRY_FLOAT);
	plan.add("slot_group", T, 3, HRY_UINT);
	plan.add("edge_class", ne, 1, HRY_UINT);
	plan.alloc(cx.device, out);
	auto dst = [&](const char *name) { return out.ptr<uint32_t>(name); };
	v.edge_class = dst("edge_class"); v.slot_group = dst("slot_group"); v.render_vertex = dst("render_vertex"); v.vertex_source = dst("vertex_source");
	v.normals = out.ptr<float>("normals"); v.ids = dst("indices"); v.ng = ng; v.nw = nw;

	if (ng) HIP_OK(hipMemsetAsync(w.count, 0, (size_t)ng * 4, st));
	if (v.nv) HIP_OK(hipMemsetAsync(w.vgroups, 0, (size_t)v.nv * 4, st));
	HIP_OK(hipMemsetAsync(w.hubs, 0, 4, st));
	timer.mark(st);
	D.ids = dst("indices");   // the numbering's ids are the buffer itself
	launch_dedup_assign(st, D, nw, w.first_slot, v.indices, v.render_vertex);
	launch_creases_normals(st, v, w);
	timer.mark(st);
	uint32_t cls[4] = {};
	HIP_OK(hipMemcpyAsync(cls, w.classes, 16, hipMemcpyDeviceToHost, st));
	HIP_OK(hipStreamSynchronize(st));
	out.device_ms = timer.ms();
	out.uploaded_bytes = 0;
	out.summary[0] = nw; out.summary[1] = ng; out.summary[2] = cls[0]; out.summary[3] = cls[1]; out.summary[4] = cls[3]; out.summary[5] = cls[2];
}

}   // namespace hry
