// Is one result the build of another?  What edges.cpp asks of a render build and shells.cpp / orient.cpp / creases.cpp / curvature.cpp of a render
// build and its edges build before a kernel reads them, and the adjacency the kernels of the last two then read (result_build.hpp).
#include <hip/hip_runtime.h>

#include "result_build.hpp"

namespace hry {

void require_render_of(const Context &cx, const Mesh &m, const RenderResult &r)
{
	if (r.block.device != cx.device) throw Error(HRY_E_ARG, "the render buffers live on another device than the context's");
	// ---- is r a render build of m?  T, nf and U as render_build computes them
	bool unweld = false;
	if (m.general) for (int g = 0; g < m.bind.nregs_face(); ++g) unweld |= m.bind.ncornerlists(g) > 0;
	const uint64_t ntri = m.ntri();
	const uint32_t nout = r.nverts;
	const NamedBuf *b_idx = r.find("indices"), *b_vsrc = r.find("vertex_source"), *b_face = r.find("tri_face"), *b_reg = r.find("face_region");
	const bool fits = b_idx && b_vsrc && b_face && r.ntris == ntri && b_idx->rows == ntri && b_idx->width == 3 && b_face->rows == ntri && b_vsrc->rows == nout &&
	                  (unweld ? (m.ne() ? nout >= 1 && nout <= m.ne() : nout == 0) : nout == m.nv) && (!m.general || (b_reg && b_reg->rows == m.nf)) &&
	                  (r.find("corner_source") != nullptr) == unweld;
	if (!fits) throw Error(HRY_E_ARG, "the render buffers are not a render build of this mesh (vertices, triangles or faces differ)");
	if (3 * ntri > (1ull << 31)) throw Error(HRY_E_UNSUPPORTED, "more than 2^31 triangle sides");
}

const float *render_positions(const Mesh &m, const RenderResult &r, const char *what, uint32_t &stride)
{
	const size_t pl = render_position_list(m, what);
	const NamedBuf *b_pos = r.find("list" + std::to_string(pl));
	const size_t at = (size_t)m.lists[pl].interp_off[0];
	if (!b_pos || b_pos->rows != r.nverts || b_pos->type != HRY_FLOAT || (size_t)b_pos->width < at + 3) throw Error(HRY_E_ARG, "the render buffers do not hold this mesh's position list");
	stride = (uint32_t)b_pos->width;
	return (const float*)b_pos->p + at;
}

const float *render_attribute(const Mesh &m, const RenderResult &r, int interp, int ncomp, const char *what, const char *noun, uint32_t &stride)
{
	auto len = [&](const AttrList &L) { return (size_t)interp < L.interp_len.size() ? L.interp_len[interp] : 0; };
	const std::string need = std::string(ncomp == 2 ? "two " : "three ") + noun + " components";
	size_t al = m.lists.size();
	if (!m.general) {
		if (m.lists.size() >= 2 && len(m.lists[1]) >= ncomp) al = 1;
	} else
		for (size_t l = 0; l < m.lists.size(); ++l) {
			if ((m.lists[l].target != 1 && m.lists[l].target != 2) || len(m.lists[l]) < ncomp) continue;
			if (al != m.lists.size()) throw Error(HRY_E_UNSUPPORTED, std::string(what) + ": several vertex or corner lists with " + need);
			al = l;
		}
	if (al == m.lists.size()) throw Error(HRY_E_UNSUPPORTED, std::string(what) + ": no vertex or corner list with " + need);
	const NamedBuf *b = r.find("list" + std::to_string(al));
	const size_t at = (size_t)m.lists[al].interp_off[interp];
	if (!b || b->rows != r.nverts || b->type != HRY_FLOAT || (size_t)b->width < at + ncomp)
		throw Error(HRY_E_ARG, std::string("the render buffers do not hold this mesh's list of ") + noun + " components");
	stride = (uint32_t)b->width;
	return (const float*)b->p + at;
}

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

dev::TriAdjacency tri_adjacency_of(const RenderResult &r, const EdgesFit &fit, const Mesh &m)
{
	auto words = [](const NamedBuf *b) { return (const uint32_t*)b->p; };
	const uint32_t T = (uint32_t)m.ntri();
	return dev::TriAdjacency{ words(r.find("indices")), words(r.find("vertex_source")), words(r.find("tri_face")), words(fit.tri_edges), words(fit.offsets),
	                          words(fit.sides), 3 * T, T, r.nverts, (uint32_t)m.nf, fit.ne };
}

}   // namespace hry
