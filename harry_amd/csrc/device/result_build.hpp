// What the builds that leave a result handle share on the host (render.cpp, edges.cpp, shells.cpp, orient.cpp, tangents.cpp,
// creases.cpp, curvature.cpp, bvh.cpp): the plan of a handle's named buffers, the timer of a build in one stretch or
// two, the one result type of the eight builds behind a render build and the checks that one build is the build of another
// (result_build.cpp).  A driver states each working buffer once -- W.take(w.field, bytes), then W.bind(base) behind the allocation
// (hip_handles.hpp: Carve) -- and fetches an output as out.ptr<T>("name") (context.hpp: DeviceResult).
#pragma once
#include "context.hpp"
#include "grow_keeping.hpp"
#include "kernels.hpp"

namespace hry {

// the named buffers of one result: add() every one while sizing, then alloc() the one block the handle owns and name its pieces
struct OutputPlan {
	struct Plan { std::string name; uint64_t rows; int width, type; size_t slot; };
	Carve O;
	std::vector<Plan> plan;
	void add(const std::string &name, uint64_t rows, int width, int type) { plan.push_back(Plan{ name, rows, width, type, O.reserve((size_t)rows * width * (type == HRY_USHORT ? 2 : 4)) }); }
	void alloc(int device, DeviceResult &out)
	{
		out.block.alloc(device, O.total);
		for (const Plan &p : plan) out.bufs.push_back(NamedBuf{ p.name, O.ptr<void>(out.block.p, p.slot), p.rows, p.width, p.type });
	}
};

// A build runs in one stretch, or in two with a few bytes coming down between them: mark() before and behind each (two marks or
// four), ms() their sum once the stream has been waited for.  The events enclose kernels only: the fills and copies lie outside them
struct StretchTimer {
	TimedEvent ev[4];
	int marks = 0;
	void mark(hipStream_t st) { HIP_OK(hipEventRecord(ev[marks++], st)); }
	double ms()
	{
		double sum = 0;
		for (int i = 0; i + 1 < marks; i += 2) {
			float stretch = 0;
			HIP_OK(hipEventElapsedTime(&stretch, ev[i], ev[i + 1]));
			sum += (double)stretch;
		}
		return sum;
	}
};

// edges.cpp, shells.cpp, orient.cpp: the builds behind a render build (include/harry_amd.h: hry_edges_build, hry_shells_build,
// hry_orient_build); the result owns its memory.  summary: E, edges with one side, with two, with more / S, closed, nonmanifold,
// misoriented shells, loops, triangles of the largest / P, orientable patches, flipped triangles, inverted patches, against edges,
// against edges remaining
struct TopologyResult : DeviceResult {
	uint64_t summary[6] = {};
	double device_ms = 0;
	uint64_t uploaded_bytes = 0;
};
typedef TopologyResult EdgesResult, ShellsResult, OrientResult;
void edges_build(Context &cx, const Mesh &m, const RenderResult &r, uint32_t flags, EdgesResult &out);   // flags: HRY_EDGES_*
void shells_build(Context &cx, const Mesh &m, const RenderResult &r, const EdgesResult &e, uint32_t flags, ShellsResult &out);   // flags: HRY_SHELLS_*
void orient_build(Context &cx, const Mesh &m, const RenderResult &r, const EdgesResult &e, uint32_t flags, OrientResult &out);   // flags: HRY_ORIENT_*
// tangents.cpp: the tangent frames of a render build (include/harry_amd.h: hry_tangents_build).  summary: framed vertices, vertices
// with a zero row, mirrored, mixed, uv-degenerate triangles, 0
typedef TopologyResult TangentsResult;
void tangents_build(Context &cx, const Mesh &m, const RenderResult &r, uint32_t flags, TangentsResult &out);   // flags: HRY_TANGENTS_*
// creases.cpp: hard edges and split normals of a render build behind its edges build with geometry (include/harry_amd.h:
// hry_creases_build).  summary: W split vertices, G groups, SMOOTH edges, SHARP edges, decoded vertices with more than one group,
// edges of the other classes
typedef TopologyResult CreasesResult;
void creases_build(Context &cx, const Mesh &m, const RenderResult &r, const EdgesResult &e, double cos_limit, uint32_t flags, CreasesResult &out);   // flags: HRY_CREASES_*
// curvature.cpp: vertex areas and curvatures of a render build behind its edges build (include/harry_amd.h: hry_curvature_build).
// summary: D decoded vertices, interior, boundary, irregular, isolated, vertices with bit 8; totals: the sums of A_d, of the angle
// defects and of H_d A_d
struct CurvatureResult : TopologyResult {
	double totals[3] = {};
};
void curvature_build(Context &cx, const Mesh &m, const RenderResult &r, const EdgesResult &e, uint32_t flags, CurvatureResult &out);   // flags: none
// bvh.cpp: the hierarchy over the triangles of a render build, the cast and the closest-point query over it (include/harry_amd.h:
// hry_bvh_build, hry_bvh_cast, hry_bvh_nearest).  summary: T, L, T - L, distinct codes, depth, 0.  The result reads nothing of the render build afterwards
typedef TopologyResult BvhResult;
void bvh_build(Context &cx, const Mesh &m, const RenderResult &r, uint32_t flags, BvhResult &out);   // flags: none
dev::BvhView bvh_view_of(const BvhResult &b);   // its seven buffers, as the kernels take them
void bvh_cast(Context &cx, const BvhResult &b, uint64_t n_rays, const float *origins, uint64_t origin_stride, const float *dirs, uint64_t dir_stride, double tmin,
              double tmax, uint32_t flags, uint32_t *hit_tri, float *hit_t, float *hit_uv, uint64_t *stat, double *device_ms);   // flags: HRY_CAST_*
void bvh_nearest(Context &cx, const BvhResult &b, uint64_t n_points, const float *points, uint64_t point_stride, double max_dist, uint32_t flags, uint32_t *near_tri,
                 double *near_d2, float *near_uv, float *near_point, uint64_t *stat, double *device_ms);   // flags: HRY_NEAREST_*
// ... and the pairs of its triangles that pass through each other (include/harry_amd.h: hry_intersections_build).  summary: T, C pairs
// of leaves whose boxes overlap, N of them that reach the segment tests, P pairs, H triangles in a pair, the box tests of the walk.
// It reads the hierarchy alone
typedef TopologyResult IntersectionsResult;
void intersections_build(Context &cx, const BvhResult &b, uint32_t flags, IntersectionsResult &out);   // flags: none

// ---- result_build.cpp
// r is a render build of m on cx's device, with at most 2^31 triangle sides: HRY_E_ARG / HRY_E_UNSUPPORTED otherwise
void require_render_of(const Context &cx, const Mesh &m, const RenderResult &r);
// the float rows of r's position list, from its first position component; stride: floats a row.  `what` as render_position_list's
const float *render_positions(const Mesh &m, const RenderResult &r, const char *what, uint32_t &stride);
// ... and of the one vertex- or corner-target list with at least ncomp components of interpretation `interp` (mixing.h ids: 16 TEX,
// 1 NORMAL), from the first of them; PLY layout: list 1.  None or several: HRY_E_UNSUPPORTED, "<what>: no / several ... <noun> components"
const float *render_attribute(const Mesh &m, const RenderResult &r, int interp, int ncomp, const char *what, const char *noun, uint32_t &stride);
// e is an edges build of (m, r) on cx's device, r a render build of m: HRY_E_ARG / HRY_E_UNSUPPORTED otherwise
struct EdgesFit { const NamedBuf *tri_edges, *offsets, *sides; uint32_t ne; };
EdgesFit require_edges_of(const Context &cx, const Mesh &m, const RenderResult &r, const EdgesResult &e);
// ... and what the kernels behind both read of them (tri_adjacency.hpp)
dev::TriAdjacency tri_adjacency_of(const RenderResult &r, const EdgesFit &fit, const Mesh &m);

}   // namespace hry
