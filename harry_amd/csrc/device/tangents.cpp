// Tangent frames of a render build, built where the render build lies in HBM (include/harry_amd.h: hry_tangents_build; kernels:
// tangents.hip; DESIGN.md "Tangents").  Nothing is uploaded: the build reads the render result's indices, the float rows of its
// position and uv lists and its "normals" -- or, with HRY_TANGENTS_STORED_NORMALS, the rows of the normal list; the mesh says which
// lists those are and what the render's sizes must be.  The decode's token and the encoder's resident mesh are left alone.
#include <hip/hip_runtime.h>

#include "result_build.hpp"

namespace hry {

using namespace dev;

void tangents_build(Context &cx, const Mesh &m, const RenderResult &r, uint32_t flags, TangentsResult &out)
{
	if (flags & ~(uint32_t)(HRY_TANGENTS_ANGLE_WEIGHTED | HRY_TANGENTS_STORED_NORMALS | HRY_TANGENTS_BITANGENTS)) throw Error(HRY_E_ARG, "unknown tangents flag");
	require_render_of(cx, m, r);
	const uint64_t ntri = m.ntri();
	const uint32_t nout = r.nverts, n = (uint32_t)(3 * ntri);
	TanView v{};
	v.indices = r.ptr<const uint32_t>("indices"); v.n = n; v.nout = nout; v.angle = (flags & HRY_TANGENTS_ANGLE_WEIGHTED) ? 1 : 0;
	v.pos = render_positions(m, r, "tangents", v.pos_stride);
	v.uv = render_attribute(m, r, 16, 2, "tangents", "texture-coordinate", v.uv_stride);
	if (flags & HRY_TANGENTS_STORED_NORMALS) v.nrm = render_attribute(m, r, 1, 3, "tangents", "normal", v.nrm_stride);
	else {
		const NamedBuf *b = r.find("normals");
		if (!b) throw Error(HRY_E_ARG, "tangents: the render build has no \"normals\" (build it with HRY_RENDER_VERTEX_NORMALS, or pass HRY_TANGENTS_STORED_NORMALS)");
		if (b->rows != nout || b->width != 3 || b->type != HRY_FLOAT) throw Error(HRY_E_ARG, "the render buffers do not hold this mesh's normals");
		v.nrm = (const float*)b->p; v.nrm_stride = 3;
	}
	HIP_OK(hipSetDevice(cx.device));

	// ---- the working buffer: per triangle its two terms and the word of its sign; per output vertex a counter and a segment start;
	// the scan's sums; the segments; the list of long segments; the four class counters
	Carve W;
	TanWork w{};
	W.take(w.terms, (size_t)ntri * 48); W.take(w.sign, (size_t)ntri * 4); W.take(w.count, (size_t)nout * 4);
	W.take(w.start, ((size_t)nout + 1) * 4); W.take(w.sums, scan_sums_words(nout) * 4); W.take(w.seg, (size_t)n * 4);
	W.take(w.hubs, ((size_t)tangents_hub_capacity(n) + 1) * 4); W.take(w.classes, 16);
	cx.d_tangents.ensure(W.total);
	W.bind(cx.d_tangents.p);

	// ---- the outputs, in one allocation
	OutputPlan plan;
	plan.add("tangents", nout, 4, HRY_FLOAT);
	if (flags & HRY_TANGENTS_BITANGENTS) plan.add("bitangents", nout, 3, HRY_FLOAT);
	plan.alloc(cx.device, out);
	v.tangents = out.ptr<float>("tangents");
	if (flags & HRY_TANGENTS_BITANGENTS) v.bitangents = out.ptr<float>("bitangents");

	hipStream_t st = cx.stream;
	StretchTimer timer;
	if (nout) HIP_OK(hipMemsetAsync(w.count, 0, (size_t)nout * 4, st));   // (the fills lie outside the events, as in render.cpp)
	HIP_OK(hipMemsetAsync(w.hubs, 0, 4, st));
	HIP_OK(hipMemsetAsync(w.classes, 0, 16, st));
	timer.mark(st);
	launch_tangents(st, v, w);
	timer.mark(st);   // (one stretch: nothing comes down in between)
	uint32_t cls[4] = {};
	HIP_OK(hipMemcpyAsync(cls, w.classes, 16, hipMemcpyDeviceToHost, st));
	HIP_OK(hipStreamSynchronize(st));
	out.device_ms = timer.ms();
	out.uploaded_bytes = 0;
	out.summary[0] = cls[0]; out.summary[1] = (uint64_t)nout - cls[0]; out.summary[2] = cls[1]; out.summary[3] = cls[2]; out.summary[4] = cls[3]; out.summary[5] = 0;
}

}   // namespace hry
