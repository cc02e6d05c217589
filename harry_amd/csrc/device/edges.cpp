// Unique edges and adjacency of a render build's triangles, built where the render build lies in HBM (include/harry_amd.h:
// hry_edges_build; kernels: dedup.hip with EdgeKey, edges.hip; DESIGN.md "Edges and adjacency").  Nothing is uploaded: the build
// reads the render result's indices, vertex_source and -- for the geometry -- the float rows of its position list; the mesh says
// which list that is and what the render's sizes must be.  The decode's token and the encoder's resident mesh are left alone.
#include <hip/hip_runtime.h>

#include "result_build.hpp"

namespace hry {

using namespace dev;

void edges_build(Context &cx, const Mesh &m, const RenderResult &r, uint32_t flags, EdgesResult &out)
{
	if (flags & ~(uint32_t)HRY_EDGES_GEOMETRY) throw Error(HRY_E_ARG, "unknown edges flag");
	const bool geometry = flags & HRY_EDGES_GEOMETRY;
	require_render_of(cx, m, r);
	const uint64_t ntri = m.ntri();
	const uint32_t nout = r.nverts;
	const uint32_t n = (uint32_t)(3 * ntri);
	uint32_t pos_stride = 0;
	const float *pos = geometry ? render_positions(m, r, "edges", pos_stride) : nullptr;
	HIP_OK(hipSetDevice(cx.device));

	// ---- the working buffer: the numbering of the sides (dedup.hip); per edge a counter (E <= 3 T of them); the scan's sums; the
	// list of long segments; the three class counters
	Carve W;
	DedupPlan D;
	D.reserve(W, n, false);   // (the ids are the output buffer tri_edges)
	uint32_t *count, *sums, *hubs, *classes;
	W.take(count, (size_t)n * 4); W.take(sums, scan_sums_words(n) * 4); W.take(hubs, ((size_t)edges_hub_capacity(n) + 1) * 4); W.take(classes, 16);
	cx.d_edges.ensure(W.total);
	W.bind(cx.d_edges.p);
	D.bind(W, cx.d_edges.p);
	hipStream_t st = cx.stream;
	StretchTimer timer;

	EdgeView u{};
	u.indices = r.ptr<const uint32_t>("indices"); u.vsrc = r.ptr<const uint32_t>("vertex_source"); u.nout = nout;
	if (n) HIP_OK(hipMemsetAsync(D.table, 0xff, D.table_bytes(), st));   // (the fills lie outside the events, as in render.cpp)
	timer.mark(st);
	if (n) launch_dedup_count(st, u, D);
	timer.mark(st);
	uint32_t ne = 0;
	if (n) HIP_OK(hipMemcpyAsync(&ne, D.total(), 4, hipMemcpyDeviceToHost, st));
	HIP_OK(hipStreamSynchronize(st));
	if (ne > n || (n && !ne)) throw Error(HRY_E_INTERNAL, "edges: the numbering does not fit the sides");

	// ---- the outputs, in one allocation
	OutputPlan plan;
	plan.add("edges", ne, 2, HRY_UINT);
	plan.add("tri_edges", ntri, 3, HRY_UINT);
	plan.add("edge_offsets", (uint64_t)ne + 1, 1, HRY_UINT);
	plan.add("edge_sides", n, 1, HRY_UINT);
	plan.add("tri_neighbours", ntri, 3, HRY_UINT);
	if (geometry) { plan.add("edge_length", ne, 1, HRY_FLOAT); plan.add("edge_cot", ne, 1, HRY_FLOAT); plan.add("edge_cos", ne, 1, HRY_FLOAT); }
	plan.alloc(cx.device, out);
	auto dst = [&](const char *name) { return out.ptr<uint32_t>(name); };

	if (ne) HIP_OK(hipMemsetAsync(count, 0, (size_t)ne * 4, st));
	HIP_OK(hipMemsetAsync(hubs, 0, 4, st));
	HIP_OK(hipMemsetAsync(classes, 0, 16, st));
	timer.mark(st);
	D.ids = dst("tri_edges");   // the numbering's ids are the buffer itself
	launch_dedup_assign(st, D, 0, nullptr);
	EdgesView v{};
	v.indices = u.indices; v.vsrc = u.vsrc; v.tri_edges = dst("tri_edges");
	v.offsets = dst("edge_offsets"); v.sides = dst("edge_sides"); v.edges = dst("edges"); v.neighbours = dst("tri_neighbours");
	v.n = n; v.nout = nout; v.ne = ne;
	if (geometry) {
		v.pos = pos; v.pos_stride = pos_stride;
		v.length = out.ptr<float>("edge_length"); v.cot = out.ptr<float>("edge_cot"); v.cos = out.ptr<float>("edge_cos");
	}
	launch_edges(st, v, count, sums, hubs, classes);
	timer.mark(st);
	uint32_t cls[3] = {};
	HIP_OK(hipMemcpyAsync(cls, classes, 12, hipMemcpyDeviceToHost, st));
	HIP_OK(hipStreamSynchronize(st));
	out.device_ms = timer.ms();
	out.uploaded_bytes = 0;
	out.summary[0] = ne; out.summary[1] = cls[0]; out.summary[2] = cls[1]; out.summary[3] = cls[2];
}

}   // namespace hry
