/*
 * harry_amd.h -- C ABI of the MI355X-native .hry codec path (libharry_amd.so).
 *
 * Drop-in boundary for the attribute-quantisation + arithmetic-coding hot path of maxvonbuelow/harry.
 * The reference has no FFI; its seams are C++ free functions.  Each entry point below names the reference
 * interface it replaces (paths relative to the reference tree):
 *
 *   hry_mesh_from_ply   <- ply::reader::read(std::istream&, mesh::Mesh&)          formats/ply/reader.cc:382-429
 *   hry_mesh_to_ply     <- ply::writer::write(std::ostream&, mesh::Mesh&, bool)   formats/ply/writer.cc:136-192
 *   hry_mesh_from_obj   <- obj::reader::read(std::istream&, const std::string&, mesh::Mesh&)  formats/obj/reader.rl:287-299
 *   hry_mesh_to_obj     <- obj::writer::write(std::ostream&, const std::string&, mesh::Mesh&) formats/obj/writer.cc:20-132
 *   hry_requant         <- quant::requant(Attrs&, const vector<Quant>&, bool)     structs/quant.h:222-242 (+ main.cc:74-91)
 *   hry_encode          <- hry::writer::write(std::ostream&, mesh::Mesh&)         formats/hry/writer.h:19, writer.cc:200-218
 *   hry_decode          <- hry::reader::read(std::istream&, mesh::Mesh&)          formats/hry/reader.h:19, reader.cc:179-193
 *   hry_bounds          <- quant::set_bounds(Attrs&)                              structs/quant.h:30-44 (called by ply/reader.cc:428)
 *   hry_render_build    (no counterpart: the mesh as render-ready device buffers, after the reference's -c dequantisation)
 *   hry_edges_build     (no counterpart: unique edges, adjacency and per-edge geometry of a render build, as device buffers)
 *   hry_shells_build    (no counterpart: connected shells of a render build, their counts, loops, area, volume and box, as device buffers)
 *   hry_orient_build    (no counterpart: which triangles of a render build to turn for a consistent winding per patch, as device buffers)
 *   hry_tangents_build  (no counterpart: a tangent frame per output vertex of a render build, from its positions, uv and normals, as device buffers)
 *   hry_creases_build   (no counterpart: hard edges at a crease limit, vertices split along them and a normal per split vertex, as device buffers)
 *   hry_curvature_build (no counterpart: mixed Voronoi area, angle defect, Gaussian and mean curvature per vertex of a render build, as device buffers)
 *   hry_bvh_build, hry_bvh_cast (no counterpart: a bounding-volume hierarchy over the triangles of a render build and closest-hit ray queries against it, on the device)
 *   hry_bvh_nearest     (no counterpart: the closest point of that hierarchy's triangles to every query point, the query behind a mesh-to-mesh deviation)
 *   hry_intersections_build (no counterpart: the pairs of that hierarchy's triangles that pass through each other, as device buffers)
 *   hry_mesh_from_device (no counterpart: hry_mesh_from_arrays from device buffers, resident for the encoder, optional exact weld)
 *   hry_mesh_from_device_corners (no counterpart: the mesh hry_mesh_from_obj builds, from device buffers: corner lists, material regions)
 *   hry_order_take      (no counterpart: the permutation between the source's numbering and the decoder's, as device tables)
 *   hry_distortion_build (no counterpart: the per-component error of a decode against its source, reduced on the device)
 *   hry_quant_sweep_build (no counterpart: that error at every quantisation width in one pass, and the width a tolerance needs)
 *   hry_rate_sweep_build (no counterpart: the coded size of the vertex attributes at every width in one pass, and the width a byte budget buys)
 *   hry_quant_sweep_build_ex / hry_distortion_normals (no counterpart: the angle a quantisation tilts each face's normal by, after the fact and at every width)
 *
 * Plain pointers and sizes only; no C++/torch types.  All functions return HRY_OK (0) or a negative error
 * code; hry_last_error() returns the message of the calling thread's last failure (the reference throws
 * std::runtime_error with the same texts, e.g. "Invalid magic number", formats/hry/reader.cc:70).
 *
 * The compute stages run as hand-written HIP kernels on gfx950.  There is no CPU fallback: without a HIP
 * device hry_ctx_create() fails with HRY_E_NODEVICE and nothing can be encoded or decoded.
 */
#ifndef HARRY_AMD_H
#define HARRY_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HRY_ABI_VERSION 6

enum {
    HRY_OK = 0,
    HRY_E_ARG = -1,         /* invalid argument */
    HRY_E_FORMAT = -2,      /* malformed PLY / .hry input */
    HRY_E_UNSUPPORTED = -3, /* valid input outside the supported subset */
    HRY_E_NODEVICE = -4,    /* no usable HIP device / HIP runtime error */
    HRY_E_NOMEM = -5,
    HRY_E_INTERNAL = -6
};

/* component types: numeric values of mixing::Type (structs/mixing.h:19), as stored in the .hry header */
enum { HRY_FLOAT = 0, HRY_DOUBLE, HRY_ULONG, HRY_LONG, HRY_UINT, HRY_INT, HRY_USHORT, HRY_SHORT, HRY_UCHAR, HRY_CHAR };

/* output profiles: COMPAT is byte-identical to the reference's single stream (v0.1);
 * CHUNKED is the version-tagged (v0.2) parallel container: same symbols, independent coder per chunk. */
enum { HRY_PROFILE_COMPAT = 0, HRY_PROFILE_CHUNKED = 1 };

typedef struct hry_ctx hry_ctx;   /* device context: HIP device, streams, workspace */
typedef struct hry_mesh hry_mesh; /* host-side mesh: flat arrays (see accessors) */

/* one -q request: list, component (-1 = every component of the list), bits (0 clears)  (main.cc:23-27,63-65) */
typedef struct hry_quant {
    int32_t list;
    int32_t comp;
    int32_t bits;
} hry_quant;

typedef struct hry_opts {
    int32_t profile;      /* HRY_PROFILE_* */
    int32_t chunk_syms;   /* CHUNKED: symbols per chunk and plane (0 = default) */
    int32_t keep_stages;  /* keep intermediate device buffers for hry_stage_get (tests) */
    int32_t flags;        /* HRY_FLAG_* */
    int32_t shard_index;  /* hry_decode of a sharded container (.hry v0.3): decode only the segments i with */
    int32_t shard_count;  /*   i % shard_count == shard_index (one process per GPU); 0 or 1 = every segment */
} hry_opts;

/* COMPAT only: the one strictly serial recurrence of the reference stream (the range register R of arith/coder.h:69-91,
 * SURVEY.md App. C-3) runs on a host core behind the device kernels (records stream down slice by slice); every parallel stage
 * stays on the device.  HRY_FLAG_DEVICE_RECURRENCE runs it on a single GPU wavefront instead (k_rchain: 8 times slower, same
 * bytes).  HRY_FLAG_HOST_RECURRENCE is accepted for older callers and changes nothing. */
#define HRY_FLAG_HOST_RECURRENCE 1
#define HRY_FLAG_DEVICE_RECURRENCE 2
/* hry_decode of a sharded container (.hry v0.3) that does not hold the whole mesh -- one rank's own part -- is an error unless this
 * flag (or a share, shard_count > 1) asks for a PARTIAL mesh: only the runs hry_mesh_runs lists are decoded, everything else is
 * filler (faces without half-edges, zero records).  The accessors read such a mesh; the writers, hry_encode, hry_mesh_upload,
 * hry_walk_run and hry_shard_plan refuse it (HRY_E_ARG). */
#define HRY_FLAG_PARTIAL 4
/* hry_encode_sharded: leave *m exactly as it is (do not store the combined bounds of the whole mesh in it) */
#define HRY_FLAG_KEEP_MESH 8

/* timings of the last hry_encode / hry_decode on this context, milliseconds */
typedef struct hry_timing {
    double host_walk_ms;   /* cut-border walk on the host (cbm/encoder.h:54-217 equivalent) */
    double h2d_ms;
    double device_ms;      /* all kernels, measured with HIP events on the codec stream */
    double d2h_ms;
    double total_ms;
    double k_rchain_ms;    /* compat: serial range recurrence kernel */
    double k_model_ms;     /* adaptive-model evaluation kernels */
    double k_predict_ms;   /* prediction + residual + symbolisation kernels; decode: candidates + chain records + the chain */
    double k_entropy_ms;   /* chunked: fused model+coder kernel */
    double k_chain_ms;     /* decode: the reconstruction chain kernels alone (k_unpredict2 / k_unpredict3) */
    uint64_t n_symbols;    /* coder invocations represented in the stream */
    uint64_t payload_bytes;
} hry_timing;

const char *hry_last_error(void);
int hry_abi_version(void);

/* ---- context ------------------------------------------------------------------------------------ */
int hry_device_count(void);   /* HIP devices this process sees (0: none) */
int hry_ctx_create(int device, hry_ctx **out);
void hry_ctx_destroy(hry_ctx *ctx);
int hry_ctx_timing(const hry_ctx *ctx, hry_timing *out);
/* the HIP stream all kernels of this context are launched on (hipStream_t as void*), for external event timing */
void *hry_ctx_stream(const hry_ctx *ctx);

/* ---- mesh (host) -------------------------------------------------------------------------------- */
int hry_mesh_from_ply(const uint8_t *ply, size_t n, hry_mesh **out);
/* Build from flat arrays: vertex records (AoS, one slot per component in its original type), polygon
 * degrees + flat vertex indices, optional face records.  Component names follow PLY conventions ("x","nx",
 * "red", ...; unknown names become named "other" interpretations, formats/ply/reader.cc:130-168). */
int hry_mesh_from_arrays(uint32_t nv, const uint8_t *vrec, int v_ncomp, const uint8_t *v_types, const char *const *v_names,
                         uint32_t nf, const uint8_t *degrees, const uint32_t *indices,
                         const uint8_t *frec, int f_ncomp, const uint8_t *f_types, const char *const *f_names,
                         hry_mesh **out);
/* flags: HRY_PLY_ASCII (the reference's --ply-ascii), HRY_PLY_PACKED: binary values of QUANTISED components in the width of the
 * storage type the header declares (a well-formed PLY).  Without it the binary writer does what the reference does: it announces
 * the storage type and dumps the whole original-width record (formats/ply/writer.cc:72-75,168) -- readable only by knowing
 * that.  `-c` (hry_requant with clear) before writing gives dequantised values in the original types instead. */
#define HRY_PLY_ASCII 1
#define HRY_PLY_PACKED 2
int hry_mesh_to_ply(const hry_mesh *m, int flags, uint8_t **out, size_t *out_len);
/* OBJ (formats/obj/reader.rl, writer.cc): positions (+ colours) per vertex; texture coordinates and normals per CORNER, shared
 * between corners; "usemtl" materials become face regions.  Such a mesh has GENERAL bindings (structs/attr.h:101-189): any
 * number of lists (hry_mesh_nlists / hry_list_target), faces and vertices belong to regions, a region names the lists its
 * elements (and, for face regions, their corners) carry, and every element holds one record index per list of its region.
 * The reader follows the reference's scanner where that differs from the OBJ specification (harry_amd/csrc/host/obj_io.cpp).
 * `dir`: where "mtllib" files are looked up (the reference passes the input path up to its last '/', formats/unified_reader.h:56).
 * hry_encode codes general bindings into the reference stream (HRY_PROFILE_COMPAT) and into the chunked container
 * (HRY_PROFILE_CHUNKED, .hry v0.2). */
int hry_mesh_from_obj(const uint8_t *obj, size_t n, const char *dir, hry_mesh **out);
int hry_mesh_to_obj(const hry_mesh *m, int flags, uint8_t **out, size_t *out_len);   /* flags: 0 */
int hry_mesh_general(const hry_mesh *m);                   /* 0: the PLY layout (list 0 = face, list 1 = vertex attributes, record i of element i) */
int hry_list_target(const hry_mesh *m, int l);             /* 0 face, 1 vertex, 2 corner, 3 none (structs/attr.h:22) */
int hry_mesh_nregions(const hry_mesh *m, int which);       /* which: 0 face regions, 1 vertex regions */
/* lists bound to region r: kind 0 = face lists, 1 = vertex lists, 2 = corner lists of face region r; returns their number */
int hry_mesh_region_lists(const hry_mesh *m, int kind, int r, uint16_t *out, int cap);
/* general bindings only: region of every face (which 0) / vertex (which 1); returns the element count */
size_t hry_mesh_regions_of(const hry_mesh *m, int which, const uint16_t **out);
/* general bindings only: record index per element and slot (kind 0 faces, 1 vertices, 2 corners = half-edges), row-major with
 * *slots entries per element; returns the element count */
size_t hry_mesh_bindings(const hry_mesh *m, int kind, const uint32_t **out, int *slots);
void hry_mesh_free(hry_mesh *m);
hry_mesh *hry_mesh_clone(const hry_mesh *m);

uint32_t hry_mesh_nv(const hry_mesh *m);
uint32_t hry_mesh_nf(const hry_mesh *m);
uint32_t hry_mesh_ne(const hry_mesh *m);
uint64_t hry_mesh_ntri(const hry_mesh *m);              /* sum(ne - 2), structs/conn.h:87 */
const uint32_t *hry_mesh_face_offsets(const hry_mesh *m); /* nf + 1 */
const uint32_t *hry_mesh_org(const hry_mesh *m);          /* ne: origin vertex of each half-edge */
const uint32_t *hry_mesh_twin(const hry_mesh *m);         /* ne: flat id of the opposite half-edge (self = border) */
int hry_mesh_nlists(const hry_mesh *m);                   /* PLY layout: 2 (list 0 = face attributes, list 1 = vertex attributes) */
int hry_list_ncomp(const hry_mesh *m, int l);
uint32_t hry_list_count(const hry_mesh *m, int l);
int hry_list_stride(const hry_mesh *m, int l);
int hry_list_type(const hry_mesh *m, int l, int c);
int hry_list_quant(const hry_mesh *m, int l, int c);
int hry_list_offset(const hry_mesh *m, int l, int c);
int hry_list_interp_ncomp(const hry_mesh *m, int l, int interp);   /* components of list l with interpretation `interp` (mixing.h ids: 0 POS, 1 NORMAL, 16 TEX); 0: none, or no such list */
int hry_list_interp_offset(const hry_mesh *m, int l, int interp);  /* the component of list l its first component of that interpretation is; -1: none, or no such list */
const uint8_t *hry_list_data(const hry_mesh *m, int l);
const uint8_t *hry_list_min(const hry_mesh *m, int l);
const uint8_t *hry_list_max(const hry_mesh *m, int l);

/* ---- codec (device) ----------------------------------------------------------------------------- */
/* min/max per component on the GPU (k_bounds); hry_mesh_from_ply leaves bounds unset until first needed */
int hry_bounds(hry_ctx *ctx, hry_mesh *m);
int hry_requant(hry_ctx *ctx, hry_mesh *m, const hry_quant *q, size_t nq, int clear);
/* Keep the mesh's attribute records and connectivity resident in HBM for subsequent hry_encode calls -- for a mesh with general
 * bindings (OBJ) its region and record tables too. */
int hry_mesh_upload(hry_ctx *ctx, hry_mesh *m);
/* mesh -> .hry.  *out is allocated by the library, release with hry_free.  The mesh's twin array is updated
 * exactly as the reference's encoder mutates it (cbm/encoder.h:150,193-198). */
int hry_encode(hry_ctx *ctx, hry_mesh *m, const hry_opts *opts, uint8_t **out, size_t *out_len);
int hry_decode(hry_ctx *ctx, const uint8_t *hry, size_t n, const hry_opts *opts, hry_mesh **out);
/* every buffer the library hands out (*out of the encoders, writers and hry_merge) goes back through hry_free and nothing else:
 * large ones belong to the library's recycling pool (their pages serve the next call), not to the C library's heap */
void hry_free(void *p);
/* host-only: what a .hry file is, without decoding it.  info[0] minor version (1 reference stream, 2 chunked, 3 sharded chunked),
 * [1] header bytes, [2] vertices, [3] faces, [4] half-edges, [5] symbols per chunk and plane (first segment; 0 for v0.1),
 * [6] the same for the connectivity planes, [7] segments (v0.3; else 1) */
int hry_container_info(const uint8_t *hry, size_t n, uint32_t info[8]);

/* ---- render-ready device buffers ---------------------------------------------------------------------------------------
 * hry_render_build turns a mesh (decoded, or read from PLY / OBJ) into buffers on ctx's device that a GPU program draws or trains
 * on.  Let U be the number of output vertices and T = hry_mesh_ntri = sum(deg - 2) triangles (structs/conn.h:87).  Buffers by name:
 *   "indices"        u32 [T, 3]  fan triangulation: triangle k of face f with corners c0 .. c(d-1) is (c0, c(k+1), c(k+2)), mapped to
 *                                output vertices; faces in mesh order
 *   "tri_face"       u32 [T]     source face of every triangle
 *   "vertex_source"  u32 [U]     decoded vertex of every output vertex
 *   "corner_source"  u32 [U]     unwelded meshes only: the first corner (half-edge) that produced the output vertex
 *   "face_region"    u16 [nf]    general bindings only: the face region (material) of every face
 *   "list<l>"        f32 [rows, ncomp(l)]  every component of list l (l in decimal: "list0", "list1", ...), row-major; vertex and
 *                                corner lists have U rows, face lists nf; lists without components or without a target are absent
 * A value of list l is (float) of what hry_requant(..., clear = 1) gives for that component (the reference's -c dequantisation,
 * structs/quant.h:98-112,215-242): lossless floats bit for bit (-0.0 included), integers as their value, quantised doubles rounded
 * once, to nearest.  An element whose region does not bind list l gets 0 in that list.
 * U depends on the input only:
 *   identity (U = nv, output vertex u = vertex u): the PLY layout, and general bindings where no face region binds a corner list;
 *   unwelded: general bindings with corner lists (OBJ vt / vn).  The key of corner c is (org[c], then for every list with corner target,
 *     in list order, the record c names, or 0xFFFFFFFF where the region of c's face does not bind that list); corners with equal keys
 *     share one output vertex, numbered in order of first occurrence over the corners in half-edge order (deterministic).
 * A partial mesh (hry_mesh_partial) is refused with HRY_E_ARG.  (Every mesh the library builds has polygons of 3 .. 255 corners:
 * the readers, hry_mesh_from_arrays and the .hry header refuse others, so T = sum(deg - 2) counts every triangle.)
 * Residency: when m is the mesh hry_decode (or hry_decode_sharded with one context) just returned on ctx and no other call has
 * touched ctx or m since, the build reads the decoded records, connectivity and binding tables where the decode left them in HBM:
 * for the PLY layout nothing goes up, in every profile (v0.1, v0.2, and a v0.3 container decoded whole on one context).  Otherwise
 * -- another context, a call in between, a mesh read from PLY / OBJ -- it uploads what it needs.  Either way the results are the
 * same, and the encoder's resident mesh (hry_mesh_upload) is left alone.
 * The handle owns its device memory: its buffers stay valid whatever later calls do on the context; free it before the context. */
typedef struct hry_render hry_render;
int hry_render_build(hry_ctx *ctx, const hry_mesh *m, hry_render **out);
uint32_t hry_render_nverts(const hry_render *r);   /* U */
uint64_t hry_render_ntris(const hry_render *r);    /* T */
/* a buffer by name: *rows (0: absent), and per row *width values of *type (HRY_UINT / HRY_USHORT / HRY_FLOAT) at device address *dev */
int hry_render_get(const hry_render *r, const char *name, const void **dev, uint64_t *rows, int *width, int *type);
/* the whole buffer to dst (device memory: dst_is_device = 1, else host memory) on ctx's stream; returns when it is there */
int hry_render_copy(hry_ctx *ctx, const hry_render *r, const char *name, void *dst, int dst_is_device);
/* device_ms: the render kernels alone, measured with HIP events (the hash table's fill and every copy lie outside);
 * uploaded_bytes: host-to-device bytes the build needed */
int hry_render_stat(const hry_render *r, double *device_ms, uint64_t *uploaded_bytes);
void hry_render_free(hry_render *r);

/* ---- normals of a render build ------------------------------------------------------------------------------------------
 * hry_render_build_ex is hry_render_build with flags; hry_render_build(ctx, m, out) is hry_render_build_ex(ctx, m, 0, out), and with
 * flags == 0 the buffers, their bytes, the kernels launched and hry_render_stat are the same.  The flags add buffers, found through
 * hry_render_get / hry_render_copy like the others and absent (rows 0) when not asked for:
 *   "normals"        f32 [U, 3]   HRY_RENDER_VERTEX_NORMALS: unit normal of the decoded vertex of every output vertex
 *   "face_normals"   f32 [nf, 3]  HRY_RENDER_FACE_NORMALS: unit normal of every face
 * Unknown flag bits, and HRY_RENDER_ANGLE_WEIGHTED without HRY_RENDER_VERTEX_NORMALS, are refused with HRY_E_ARG.
 * Positions: P[v] = the first three components of interpretation POS (mixing.h id 0) of the vertex-target list, as the floats the
 *   build's "list<l>" buffer holds for that vertex (after the -c dequantisation; lossless floats bit for bit), widened to double.  PLY
 *   layout: list 1.  General bindings: the one vertex-target list with at least three POS components, which every vertex region must
 *   bind.  Fewer than three position components, several such lists, or a vertex region that binds none: HRY_E_UNSUPPORTED with a
 *   text that says which; *out stays NULL and ctx stays usable.  A partial mesh is refused as by hry_render_build.  Normals a file
 *   stored (nx ny nz, OBJ vn) stay in their "list<l>"; they are not read here.
 * Arithmetic: every operation is an individually rounded IEEE double operation, in the written order.
 *   N_f = sum over k = 1 .. d-2 of (P[c_k] - P[c_0]) x (P[c_(k+1)] - P[c_0]) for face f with corners c_0 .. c_(d-1): the cross products
 *     of the fan triangles of "indices", relative to c_0 (a mesh far from the origin does not cancel); a x b = (a.y b.z - a.z b.y,
 *     a.z b.x - a.x b.z, a.x b.y - a.y b.x); |a| = sqrt((a.x a.x + a.y a.y) + a.z a.z).
 *   face_normals[f] = (float)(N_f / |N_f|) per component; where |N_f| is 0 or not finite the row is (0, 0, 0) and the face
 *     contributes nothing to any vertex.
 *   S_v, area weights (default): the sum of N_f over the corners c with org[c] == v, f the face of c.
 *   S_v, HRY_RENDER_ANGLE_WEIGHTED: the sum of theta_c * (N_f / |N_f|), theta_c = atan2(|a x b|, a . b) with a = P[next corner] - P[v]
 *     and b = P[previous corner] - P[v] within the face, a . b = (a.x b.x + a.y b.y) + a.z b.z.
 *   normals[u] = (float)(S_v / |S_v|) for v = vertex_source[u], (0, 0, 0) where |S_v| is 0 or not finite (an isolated vertex, a NaN
 *     position, exactly opposed faces).  Output vertices of one decoded vertex get the same bits: the unweld does not crease shading.
 * Determinism: the bits of both buffers depend on the mesh alone -- not on the run, on residency, or on the order atomics complete
 *   in (there are no floating-point atomics).  A vertex's sum starts from +0 and runs over its corners in ascending half-edge id, one
 *   after the other.  A vertex with more than 32 corners (n of them) instead sums 256 consecutive ranges of ceil(n / 256) corners each in
 *   that way and adds the 256 partial sums in range order: an association n alone determines.  All of it runs on the device.
 * The timing of hry_render_stat encloses the normals' kernels. */
#define HRY_RENDER_VERTEX_NORMALS 1u   /* buffer "normals"      f32 [U, 3]  */
#define HRY_RENDER_FACE_NORMALS   2u   /* buffer "face_normals" f32 [nf, 3] */
#define HRY_RENDER_ANGLE_WEIGHTED 4u   /* vertex normals weighted by corner angle instead of face area */
int hry_render_build_ex(hry_ctx *ctx, const hry_mesh *m, uint32_t flags, hry_render **out);

/* ---- edges and adjacency of a render build -------------------------------------------------------------------------------
 * hry_edges_build derives, on ctx's device, what a consumer of "indices" derives next: the unique edges, the triangles that meet at
 * each, the triangle across each side and -- with HRY_EDGES_GEOMETRY -- length, cotangent weight and the cosine between the two
 * triangles.  r is a render build of m on ctx's device; the build reads r's "indices", "vertex_source" and position list where they
 * lie in HBM: nothing is uploaded (uploaded_bytes is 0), the handle owns its memory like the other results, and r may be freed
 * afterwards.  Let T be the triangles, I = indices, vs = vertex_source.
 * Sides: side s = 3 t + k (k = 0, 1, 2) of triangle t joins I[t][k] to I[t][(k + 1) % 3].  Its key is the unordered pair of DECODED
 *   vertices { vs[I[t][k]], vs[I[t][(k + 1) % 3]] }: a uv or normal seam of an unwelded mesh is one edge, not two boundaries (in the
 *   PLY layout vs is the identity).  No side is left out: one whose two ends are the same decoded vertex is an edge like any other.
 * Edges are numbered in order of the first side of their key, ascending s: deterministic, whatever order atomics complete in.
 * Buffers by name, E = hry_edges_count:
 *   "edges"           u32 [E, 2]  the output vertices of the edge's first side, ordered so that vs[row[0]] <= vs[row[1]] (ties keep
 *                                 the side's order)
 *   "tri_edges"       u32 [T, 3]  the edge of side (t, k)
 *   "edge_offsets"    u32 [E + 1] CSR offsets into "edge_sides"
 *   "edge_sides"      u32 [3 T]   the sides of edge e, in ascending s, at [edge_offsets[e], edge_offsets[e + 1])
 *   "tri_neighbours"  u32 [T, 3]  the triangle of the other side where the edge of side (t, k) has exactly two sides, else HRY_NO_ELEMENT
 * and with HRY_EDGES_GEOMETRY, from P[u] = the first three position components of output vertex u, read as the floats of r's
 * "list<l>" buffer and widened to double (l: the position list by the rule of the normals above, with the same HRY_E_UNSUPPORTED
 * refusals); every operation an individually rounded IEEE double operation in the written order, a . b = (a.x b.x + a.y b.y) + a.z b.z,
 * a x b and |a| as in the normals' contract, no floating-point atomics:
 *   "edge_length"     f32 [E]     (float)|P[b] - P[a]| for edges[e] = (a, b)
 *   "edge_cot"        f32 [E]     (float)(0.5 * S): S starts from +0 and adds, over the edge's sides in ascending s, one after the other,
 *                                 c = (u . v) / |u x v| with u = P[from] - P[o], v = P[to] - P[o], o the triangle's third corner; c counts
 *                                 as 0 where |u x v| is 0 or not finite, or where c is not finite
 *   "edge_cos"        f32 [E]     an edge with exactly two sides s0 < s1 in triangles t0, t1: (float)(n_t0 . n_t1), N_t = (P1 - P0) x (P2 - P0),
 *                                 n_t = N_t / |N_t| per component; negated when both sides run from the same decoded vertex to the same
 *                                 decoded vertex (the triangles are wound against each other).  Exactly 2.0f ("none") where the edge does
 *                                 not have two sides, or where either |N_t| is 0 or not finite
 * The sum of a long segment is the same plain left-to-right one: the bits depend on r alone.
 * Refusals: null arguments, unknown flag bits, an r whose U / T / nf do not fit m or that lives on another device: HRY_E_ARG; 3 T > 2^31:
 * HRY_E_UNSUPPORTED; *out stays NULL and ctx stays usable.
 *   hry_edges_get / _copy / _stat  as hry_render_get / _copy / _stat (an absent or empty buffer: *rows 0, *dev NULL; _copy refuses a
 *                        context on another device); device_ms: the kernels, by events
 *   hry_edges_summary    out = { E, edges with one side (boundary), with two (manifold), with more }: a device reduction over
 *                        "edge_offsets" during the build, no buffer is downloaded for it */
typedef struct hry_edges hry_edges;
#define HRY_EDGES_GEOMETRY 1u   /* buffers "edge_length", "edge_cot", "edge_cos" f32 [E] */
int hry_edges_build(hry_ctx *ctx, const hry_mesh *m, const hry_render *r, uint32_t flags, hry_edges **out);
uint64_t hry_edges_count(const hry_edges *e);                     /* E */
int hry_edges_get(const hry_edges *e, const char *name, const void **dev, uint64_t *rows, int *width, int *type);
int hry_edges_copy(hry_ctx *ctx, const hry_edges *e, const char *name, void *dst, int dst_is_device);
int hry_edges_summary(const hry_edges *e, uint64_t out[4]);
int hry_edges_stat(const hry_edges *e, double *device_ms, uint64_t *uploaded_bytes);
void hry_edges_free(hry_edges *e);

/* ---- shells of a render build ----------------------------------------------------------------------------------------------
 * hry_shells_build derives, on ctx's device, the connected pieces of the triangles and what is asked of each next: its counts, its
 * boundary loops and -- with HRY_SHELLS_GEOMETRY -- area, signed volume and box.  r is a render build of m and e an edges build of
 * (m, r), both on ctx's device; the build reads r's "indices", "vertex_source", "tri_face" and e's "tri_edges", "edges",
 * "edge_offsets", "edge_sides" where they lie in HBM, with geometry also the float rows of r's position list: nothing is uploaded
 * (uploaded_bytes is 0), the handle owns its memory like the other results, and r and e may be freed afterwards.  Let T be the
 * triangles, I = indices, vs = vertex_source, E = hry_edges_count(e).
 * Shells: two triangles belong to one shell when a chain of triangles joins them in which consecutive ones have a side on the same
 *   edge of e.  An edge with two or more sides joins all its sides, non-manifold ones included; sharing only a vertex does not join
 *   (two spheres touching at a point are two shells).  Edges are keyed by DECODED vertices, so a uv or normal seam does not cut a
 *   shell.  Shells are numbered by their lowest triangle, ascending: shell 0 holds triangle 0; deterministic, whatever order atomics
 *   complete in.  Isolated vertices belong to no shell.
 * Buffers by name, S = hry_shells_count:
 *   "tri_shell"       u32 [T]     the shell of every triangle
 *   "face_shell"      u32 [nf]    the shell of every face (its fan triangles share their diagonals: one shell); HRY_NO_ELEMENT for a
 *                                 face without a triangle
 *   "edge_shell"      u32 [E]     the shell of the edge's sides
 *   "shell_first"     u32 [S]     the shell's lowest triangle
 *   "shell_counts"    u32 [S, 8]  triangles, faces, vertices, edges, boundary, nonmanifold, misoriented, loops:
 *                                 vertices: the distinct DECODED vertices vs[I[t][k]] its triangles name (a vertex where two shells
 *                                 touch counts in both); boundary: its edges with one side; nonmanifold: with more than two;
 *                                 misoriented: with exactly two sides that both run from the same decoded vertex to the same decoded
 *                                 vertex (the condition under which "edge_cos" is negated); loops: the components of its boundary
 *                                 edges, two of them joined where they share a decoded vertex -- on a manifold shell the number of
 *                                 boundary cycles.  Boundary edges of different shells are never joined, also where the shells touch
 *   Euler number of a row: vertices - edges + triangles.  (The "Topology:" line of the command line prints V - E + FACES over the
 *   whole mesh, which differs on polygon meshes.)  Genus of a row with nonmanifold = 0 and misoriented = 0:
 *   (2 - euler - loops) / 2; other rows have none.
 * and with HRY_SHELLS_GEOMETRY, from P[u] = the position of output vertex u, read as for the edges' geometry (the same list, the same
 * HRY_E_UNSUPPORTED refusals) and widened to double; every operation an individually rounded IEEE double operation in the written
 * order, a . b, a x b and |a| as in the edges' and normals' contracts, no floating-point atomics:
 *   "shell_measures"  f32 [S, 8]  area, signed volume, min x, min y, min z, max x, max y, max z
 *     area   = (float)(0.5 * sum of |(P1 - P0) x (P2 - P0)|), Pk = P[I[t][k]], over the shell's triangles
 *     volume = (float)(sum of a . (b x c) / 6 -- the sum divided once), a, b, c = P0 - O, P1 - O, P2 - O with O = P[I[shell_first][0]]:
 *              a mesh far from the origin does not cancel.  Positive for a closed shell whose triangles are wound counter-clockwise
 *              seen from outside
 *     A term that is not finite counts as +0.  Order of the sums: chunk c is the triangles [256 c, 256 c + 256); the shell's partial of
 *     a chunk starts from +0 and adds the terms of its triangles in the chunk in ascending t; the shell's sum starts from +0 and adds
 *     the partials of the chunks that hold one of its triangles in ascending c.  The bits depend on (r, e) alone.
 *     box: per coordinate the least and greatest FINITE float over the output vertices the shell's triangles name, -0 below +0; a
 *     coordinate without a finite value gets +inf and -inf
 * T = 0: S = 0 and every buffer is empty.
 * Refusals: null arguments, unknown flag bits, an r or e that does not fit (T, nf, U, E, rows of "tri_edges" / "edge_offsets" /
 * "edge_sides") or lives on another device: HRY_E_ARG; geometry without three position components: HRY_E_UNSUPPORTED; *out stays
 * NULL and ctx stays usable.
 *   hry_shells_get / _copy / _stat  as hry_edges_get / _copy / _stat
 *   hry_shells_summary   out = { S, closed shells (boundary = 0 and nonmanifold = 0), shells with nonmanifold > 0, shells with
 *                        misoriented > 0, loops over all shells, triangles of the largest shell }: device reductions during the
 *                        build, no buffer is downloaded for them */
typedef struct hry_shells hry_shells;
#define HRY_SHELLS_GEOMETRY 1u   /* buffer "shell_measures" f32 [S, 8] */
int hry_shells_build(hry_ctx *ctx, const hry_mesh *m, const hry_render *r, const hry_edges *e, uint32_t flags, hry_shells **out);
uint64_t hry_shells_count(const hry_shells *s);                   /* S */
int hry_shells_get(const hry_shells *s, const char *name, const void **dev, uint64_t *rows, int *width, int *type);
int hry_shells_copy(hry_ctx *ctx, const hry_shells *s, const char *name, void *dst, int dst_is_device);
int hry_shells_summary(const hry_shells *s, uint64_t out[6]);
int hry_shells_stat(const hry_shells *s, double *device_ms, uint64_t *uploaded_bytes);
void hry_shells_free(hry_shells *s);

/* ---- a consistent winding per patch of a render build --------------------------------------------------------------------------
 * hry_orient_build says, on ctx's device, which triangles to turn so that neighbours agree, which pieces cannot be oriented at all
 * and -- with HRY_ORIENT_OUTWARD -- which way is outward.  r is a render build of m and e an edges build of (m, r), both on ctx's
 * device; the build reads r's "indices", "vertex_source", "tri_face" and e's "tri_edges", "edge_offsets", "edge_sides" where they lie
 * in HBM, with OUTWARD also the float rows of r's position list: nothing is uploaded (uploaded_bytes is 0), the handle owns its
 * memory like the other results, and r and e may be freed afterwards.  Let T be the triangles, I = indices, vs = vertex_source.
 * Joining edge: an edge of e with exactly two sides, in two different triangles, whose two ends are different decoded vertices.  It
 *   is AGAINST when both sides run from the same decoded vertex to the same decoded vertex (the shells' "misoriented" condition),
 *   else ALONG.  Edges with one side or more than two, and edges whose ends coincide, relate nothing.
 * Same-face rule: triangles t and t + 1 with the same tri_face are always related ALONG, whatever their diagonal's edge looks like:
 *   a face never splits and one flip per face is well defined.
 * Patches: two triangles are in one patch when a chain of joining edges and same-face relations connects them.  Patches are
 *   numbered by their lowest triangle, ascending: patch 0 holds triangle 0; deterministic, whatever order atomics complete in.  A
 *   patch is a subset of a shell: non-manifold edges join shells but not patches.
 * Orientable: a patch whose triangles can be given flips f[t] in {0, 1} with f[t0] ^ f[t1] = (against ? 1 : 0) over every relation.
 *   The relative flips put f = 0 at the patch's lowest triangle.  A patch that is not orientable (a Moebius strip, a Klein bottle)
 *   has f = 0 everywhere.
 * HRY_ORIENT_MAJORITY: in an orientable patch with 2 * flipped > triangles every f is inverted; on a tie the lowest triangle keeps
 *   its winding.
 * HRY_ORIENT_OUTWARD: needs three position components -- P[u], the position of output vertex u, read as for the edges' geometry (the
 *   same list, the same HRY_E_UNSUPPORTED refusals).  Applied after MAJORITY: an orientable patch with open = 0 whose float volume
 *   (below) is < 0 is inverted; a volume of 0 or NaN leaves it.
 * Buffers by name, P = hry_orient_count:
 *   "tri_patch"         u32 [T]     the patch of every triangle
 *   "tri_flip"          u32 [T]     0 / 1, final
 *   "face_flip"         u32 [nf]    the flip of the face's triangles; 0 for a face without a triangle
 *   "oriented_indices"  u32 [T, 3]  I[t], or (I[t][0], I[t][2], I[t][1]) where tri_flip[t]
 *   "patch_first"       u32 [P]     the patch's lowest triangle
 *   "patch_counts"      u32 [P, 8]  triangles, faces, flipped (triangles, final), flipped_faces, against (joining edges that are
 *                                   against in the source), open (sides of its triangles whose edge is not a joining edge),
 *                                   orientable (0 / 1), inverted (0 / 1: turned as a whole by OUTWARD)
 * and with HRY_ORIENT_OUTWARD:
 *   "patch_measures"    f32 [P, 8]  area, signed volume, min x, min y, min z, max x, max y, max z: "shell_measures" of
 *                                   hry_shells_build word for word, with patches for shells -- the same double operations, the
 *                                   same chunks of 256 triangles, the same order of the sums, the same box.  Before the outward step
 *                                   it reads the triangles as "oriented_indices" (relative flips, then majority if asked);
 *                                   O = P[corner 0 of the patch's lowest triangle], which a flip leaves unchanged.  The volume of an
 *                                   inverted patch is then negated, which is exact
 * T = 0: P = 0 and every buffer is empty.
 * Refusals: null arguments, unknown flag bits, an r or e that does not fit (as hry_shells_build) or lives on another device:
 * HRY_E_ARG; OUTWARD without three position components: HRY_E_UNSUPPORTED; *out stays NULL and ctx stays usable.
 *   hry_orient_get / _copy / _stat  as hry_shells_get / _copy / _stat
 *   hry_orient_summary   out = { P, orientable patches, flipped triangles, inverted patches, against edges, against edges
 *                        remaining (those in patches that are not orientable) }: device reductions during the build, no buffer is
 *                        downloaded for them */
typedef struct hry_orient hry_orient;
#define HRY_ORIENT_MAJORITY 1u   /* the smaller side of every orientable patch is flipped */
#define HRY_ORIENT_OUTWARD  2u   /* closed orientable patches enclose a positive volume; buffer "patch_measures" f32 [P, 8] */
int hry_orient_build(hry_ctx *ctx, const hry_mesh *m, const hry_render *r, const hry_edges *e, uint32_t flags, hry_orient **out);
uint64_t hry_orient_count(const hry_orient *o);                   /* P */
int hry_orient_get(const hry_orient *o, const char *name, const void **dev, uint64_t *rows, int *width, int *type);
int hry_orient_copy(hry_ctx *ctx, const hry_orient *o, const char *name, void *dst, int dst_is_device);
int hry_orient_summary(const hry_orient *o, uint64_t out[6]);
int hry_orient_stat(const hry_orient *o, double *device_ms, uint64_t *uploaded_bytes);
void hry_orient_free(hry_orient *o);

/* ---- tangent frames of a render build ---------------------------------------------------------------------------------------
 * hry_tangents_build computes, on ctx's device, what a renderer needs before it can shade a textured mesh with a normal map: a
 * tangent and a handedness per OUTPUT vertex.  r is a render build of m on ctx's device; the build reads r's "indices", the float
 * rows of its position and uv lists and its "normals" (or, with HRY_TANGENTS_STORED_NORMALS, of its normal list) where they lie in
 * HBM: nothing is uploaded (uploaded_bytes is 0), the handle owns its memory like the other results, and r may be freed afterwards.
 * Let T be the triangles, U the output vertices, I = indices.
 * Buffers by name:
 *   "tangents"    f32 [U, 4]  (t.x, t.y, t.z, w): the unit tangent and the handedness, +1 or -1; (0, 0, 0, 0): no frame
 *   "bitangents"  f32 [U, 3]  HRY_TANGENTS_BITANGENTS: w * (n x t); (0, 0, 0) where the tangent row is zero
 * Inputs:
 *   P[u]: the position of output vertex u, read as for the edges' geometry (the same list, the same HRY_E_UNSUPPORTED refusals).
 *   uv[u]: the first two components of interpretation TEX (mixing.h id 16; PLY u v / tu tv, OBJ vt) of output vertex u, read as the
 *     floats of r's "list<l>" buffer and widened to double.  l: the one vertex- or corner-target list with at least two TEX
 *     components; in the PLY layout list 1, when it has them.  No such list, or several: HRY_E_UNSUPPORTED with a text that says
 *     which.  An element whose region does not bind the list reads 0 there (as every "list<l>").
 *   n[u]: the float row of r's "normals" -- a render build without it is refused with HRY_E_ARG and a text that names
 *     HRY_RENDER_VERTEX_NORMALS -- or, with HRY_TANGENTS_STORED_NORMALS, the first three components of interpretation NORMAL (id 1;
 *     PLY nx ny nz, OBJ vn) of the one vertex- or corner-target list that has three (none, or several: HRY_E_UNSUPPORTED).  Either
 *     way the row is widened to double and divided by its length, per component, in double.
 * Arithmetic: every operation is an individually rounded IEEE double operation, in the written order; a . b, a x b and |a| as in the
 *   edges' and normals' contracts; there are no floating-point atomics.
 * Per triangle t = (i0, i1, i2) of I:
 *   e1 = P[i1] - P[i0], e2 = P[i2] - P[i0]; (a1, b1) = uv[i1] - uv[i0], (a2, b2) = uv[i2] - uv[i0];
 *   det = a1 b2 - a2 b1; Tr = e1 b2 - e2 b1 and Br = e2 a1 - e1 a2, per component; both negated where det < 0.
 *   The triangle is uv-degenerate, and contributes to no vertex, where det is 0 or not finite, where a component of Tr or Br is not
 *   finite or, with HRY_TANGENTS_ANGLE_WEIGHTED, where |Tr| or |Br| is 0.  (A triangle of an element that binds no uv reads equal
 *   uv at its corners: det is 0.)
 *   Its terms at each of its three corners: Tr and Br themselves (default: uv-area weights, the counterpart of the normals' N_f), or
 *   with HRY_TANGENTS_ANGLE_WEIGHTED theta * (Tr / |Tr|) and theta * (Br / |Br|), the quotients per component, theta =
 *   atan2(|a x b|, a . b) with a = P[next corner] - P[corner], b = P[previous corner] - P[corner] within the triangle.
 * Per output vertex u -- not per decoded vertex: a uv seam splits the frame, unlike the normals:
 *   S_T and S_B start from +0 and add the terms of the index slots s = 3 t + k with I[t][k] == u, in ascending s, one after the other.
 *   A vertex with more than 32 slots (n of them) instead sums 256 consecutive ranges of ceil(n / 256) slots each in that way and adds
 *   the 256 partial sums in range order, as the normals do: an association n alone determines.
 *   R = S_T - n (n . S_T) per component (the product first); t = R / |R|; w = -1 where (n x t) . S_B < 0, else +1.
 *   tangents[u] = ((float)t, (float)w); bitangents[u] = (float)(w * (n x t)) per component.  Both rows are zeros where no triangle
 *   contributed (an isolated vertex, uv-degenerate triangles only), or where |n| or |R| is 0 or not finite.
 * Determinism: the bits of both buffers depend on r alone -- not on the run, on residency, or on the order atomics complete in.
 * Refusals: null arguments, unknown flag bits, an r whose U / T / nf do not fit m or that lives on another device: HRY_E_ARG; 3 T > 2^31:
 * HRY_E_UNSUPPORTED; *out stays NULL and ctx stays usable.
 *   hry_tangents_count   output vertices that got a frame
 *   hry_tangents_get / _copy / _stat  as hry_edges_get / _copy / _stat
 *   hry_tangents_summary out = { framed vertices, vertices with a zero row, framed vertices with w = -1 (mirrored uv), vertices whose
 *                        contributing triangles have both signs of det (mixed: the frame averages across a mirror seam),
 *                        uv-degenerate triangles, 0 (reserved) }: device reductions during the build, no buffer is downloaded for them */
typedef struct hry_tangents hry_tangents;
#define HRY_TANGENTS_ANGLE_WEIGHTED 1u  /* unit directions weighted by the corner's angle instead of uv-area weights */
#define HRY_TANGENTS_STORED_NORMALS 2u  /* n from the file's normal list (nx ny nz / OBJ vn) instead of r's "normals" */
#define HRY_TANGENTS_BITANGENTS     4u  /* also buffer "bitangents" f32 [U, 3] */
int hry_tangents_build(hry_ctx *ctx, const hry_mesh *m, const hry_render *r, uint32_t flags, hry_tangents **out);
uint64_t hry_tangents_count(const hry_tangents *t);               /* output vertices that got a frame */
int hry_tangents_get(const hry_tangents *t, const char *name, const void **dev, uint64_t *rows, int *width, int *type);
int hry_tangents_copy(hry_ctx *ctx, const hry_tangents *t, const char *name, void *dst, int dst_is_device);
int hry_tangents_summary(const hry_tangents *t, uint64_t out[6]);
int hry_tangents_stat(const hry_tangents *t, double *device_ms, uint64_t *uploaded_bytes);
void hry_tangents_free(hry_tangents *t);

/* ---- hard edges and split normals of a render build ---------------------------------------------------------------------------
 * The normals of a render build are smooth everywhere: one per decoded vertex.  hry_creases_build takes a crease limit, splits every
 * vertex where the surface folds more sharply than that, and gives each split vertex the normal of its own smooth fan -- on ctx's
 * device.  r is a render build of m; e is an edges build of r WITH HRY_EDGES_GEOMETRY (without it: HRY_E_ARG, and the text names
 * the flag).  The build reads r's "indices", "vertex_source", "tri_face" and the float rows of its position list, and e's
 * "edge_offsets", "edge_sides" and "edge_cos", where they lie in HBM: nothing is uploaded (uploaded_bytes is 0), the handle owns one
 * allocation like the other results, and r and e may be freed afterwards.
 * Let T be the triangles, U the output vertices of r, E the edges, I = indices, vs = vertex_source; slot s = 3 t + k is corner k of
 * triangle t, and side s runs from I[s] to the next corner of t.  P[u], a . b, a x b and |a| as in the edges' contract (the same
 * position list, the same HRY_E_UNSUPPORTED refusals).  Every floating-point operation is an individually rounded IEEE double
 * operation, in the written order; there are no floating-point atomics.
 * The limit is a cosine, not an angle, so that the decision is exact at equality: a cube's edge_cos is exactly 0, while
 * cos(radians(90)) is 6.1e-17.  cos_limit must not be NaN (HRY_E_ARG); every other value is legal: <= -1 makes every eligible edge
 * smooth, > 1 makes every real edge sharp (flat shading).
 * Buffers by name:
 *   "edge_class"     u32 [E]     HRY_CREASE_*.  The first rule that applies:
 *                                  BOUNDARY     the edge has one side
 *                                  NONMANIFOLD  it has more than two
 *                                  DEGENERATE   both ends of its first side are the same decoded vertex
 *                                  MISORIENTED  both sides run from the same decoded vertex to the same decoded vertex
 *                                  SMOOTH       both sides have the same tri_face: a fan diagonal of a polygon is never a crease
 *                                  DEGENERATE   edge_cos is exactly 2.0f (a side's triangle has no normal)
 *                                  SMOOTH       where (double)edge_cos[e] >= cos_limit, else SHARP
 *   "slot_group"     u32 [T, 3]  the smooth group of every slot.  Across a SMOOTH edge with sides p < q, and for each of its two
 *                                decoded end vertices v, the slot of p at v is united with the slot of q at v; the slot of side
 *                                3 t + k at v is 3 t + k if vs[I[t][k]] == v, else 3 t + (k + 1) % 3.  Nothing else unites slots.
 *                                A group is named by its smallest slot; groups are numbered 0 .. G-1 by ascending smallest slot
 *   "indices"        u32 [T, 3]  the split vertex of every slot.  The key of slot s is (I[s], group of s); slots with equal keys
 *                                share one split vertex; split vertices are numbered 0 .. W-1 by first occurrence over ascending s
 *   "render_vertex"  u32 [W]     the output vertex of r a split vertex stands for: any "list<l>" row of r follows by a gather
 *   "vertex_source"  u32 [W]     its decoded vertex, vs[render_vertex[w]]
 *   "normals"        f32 [W, 3]  (float)(S_g / |S_g|) per component, g the group of w's slots; zeros where |S_g| is 0 or not finite
 * A uv seam inside a smooth group therefore still gives two split vertices -- I differs -- with the same normal bits: the unweld
 * does not crease shading, only the limit does.
 * The term of slot (t, k): N_t = (P[I[t][1]] - P[I[t][0]]) x (P[I[t][2]] - P[I[t][0]]) (default: area weights), or with
 * HRY_CREASES_ANGLE_WEIGHTED theta * (N_t / |N_t|), the quotient and the product per component, theta = atan2(|a x b|, a . b) with
 * a = P[next corner] - P[corner], b = P[previous corner] - P[corner] within the triangle.  A triangle whose |N_t| is 0 or not finite
 * contributes nothing.
 * S_g starts from +0 and adds the terms of the group's slots in ascending s, one after the other.  A group of more than 32 slots (n
 * of them) instead sums 256 consecutive ranges of ceil(n / 256) slots each in that way and adds the 256 partial sums in range
 * order, as the normals do: an association n alone determines.
 * (Where everything is smooth -- an oriented manifold triangle mesh and cos_limit <= -1 -- W = U, render_vertex is a permutation,
 * render_vertex[indices] is r's "indices" -- equal to "indices" itself where r's vertices are numbered by first use -- and
 * normals[w] has the bits of HRY_RENDER_VERTEX_NORMALS' row render_vertex[w] with the same weights.)
 * Determinism: the bits of every buffer depend on r, e, cos_limit and the flags alone -- not on the run, on residency, or on the
 * order atomics complete in.
 * Refusals: null arguments, unknown flag bits, a NaN limit, an r or e that does not fit m or each other (U / T / nf / E) or that
 * lives on another device, an e without geometry: HRY_E_ARG; 3 T > 2^31: HRY_E_UNSUPPORTED; *out stays NULL and ctx stays usable.
 * Out of scope: writing split normals into an OBJ or PLY, a tangents build over split vertices, and crease-aware terms per polygon
 * (the terms are the fan triangles').
 *   hry_creases_count    W, the split vertices
 *   hry_creases_get / _copy / _stat  as hry_edges_get / _copy / _stat
 *   hry_creases_summary  out = { W, G, SMOOTH edges, SHARP edges, decoded vertices with more than one group, edges of the classes
 *                        BOUNDARY .. DEGENERATE }: device reductions during the build, no buffer is downloaded for them */
typedef struct hry_creases hry_creases;
#define HRY_CREASES_ANGLE_WEIGHTED 1u   /* terms weighted by the corner's angle instead of triangle area */
#define HRY_CREASE_SMOOTH      0u
#define HRY_CREASE_SHARP       1u
#define HRY_CREASE_BOUNDARY    2u
#define HRY_CREASE_NONMANIFOLD 3u
#define HRY_CREASE_MISORIENTED 4u
#define HRY_CREASE_DEGENERATE  5u
int hry_creases_build(hry_ctx *ctx, const hry_mesh *m, const hry_render *r, const hry_edges *e, double cos_limit, uint32_t flags, hry_creases **out);
uint64_t hry_creases_count(const hry_creases *c);                 /* W: split output vertices */
int hry_creases_get(const hry_creases *c, const char *name, const void **dev, uint64_t *rows, int *width, int *type);
int hry_creases_copy(hry_ctx *ctx, const hry_creases *c, const char *name, void *dst, int dst_is_device);
int hry_creases_summary(const hry_creases *c, uint64_t out[6]);
int hry_creases_stat(const hry_creases *c, double *device_ms, uint64_t *uploaded_bytes);
void hry_creases_free(hry_creases *c);

/* ---- vertex areas and curvatures of a render build ------------------------------------------------------------------------------
 * hry_curvature_build computes, on ctx's device, the discrete operators of Meyer, Desbrun, Schroeder and Barr per vertex: the mixed
 * Voronoi area, the angle defect, the Gaussian curvature, the mean curvature vector and the mean curvature -- what "edge_cot" of the
 * edges build is the weight of.  r is a render build of m; e is an edges build of r (HRY_EDGES_GEOMETRY is not needed).  The build
 * reads r's "indices", "vertex_source" and the float rows of its position list, and e's "edge_offsets" and "edge_sides", where they
 * lie in HBM: nothing is uploaded (uploaded_bytes is 0), the handle owns one allocation like the other results, and r and e may be
 * freed afterwards.  flags must be 0.
 * Let T be the triangles, U the output vertices of r, D = the decoded vertices of m, I = indices, vs = vertex_source; slot s = 3 t + k
 * is corner k of triangle t and belongs to decoded vertex vs[I[t][k]].  P[u], a . b, a x b and |a| as in the edges' contract (the
 * same position list, the same HRY_E_UNSUPPORTED refusals).  Every floating-point operation is an individually rounded IEEE double
 * operation, in the written order; sums of products are evaluated left to right; there are no floating-point atomics.
 * At slot s = 3 t + k, within triangle t:
 *   o = P[I[t][k]], a = P[I[t][(k + 1) % 3]] - o, b = P[I[t][(k + 2) % 3]] - o;
 *   x_k = |a x b|, d_k = a . b, c_k = d_k / x_k, counted as 0 where x_k is 0 or not finite or where c_k is not finite (the rule of
 *   "edge_cot").  N_t = (P[I[t][1]] - P[I[t][0]]) x (P[I[t][2]] - P[I[t][0]]).
 *   A triangle whose |N_t| is 0 or not finite contributes no terms at any of its slots.  A fan diagonal of a polygon is an edge like
 *   any other: the quantities are those of the triangles as rendered.
 * The terms of a slot of a usable triangle (indices of c are corners modulo 3: the angle opposite edge a is at corner k + 2):
 *   angle        theta_s = atan2(x_k, d_k)
 *   mixed area   with area_t = 0.5 * |N_t|: where any of d_0, d_1, d_2 is < 0 (an obtuse triangle), A_s = 0.5 * area_t where
 *                d_k < 0 and 0.25 * area_t otherwise; else A_s = 0.125 * ((a . a) * c_{k+2} + (b . b) * c_{k+1})
 *   Laplace      L_s = -(c_{k+2} * a + c_{k+1} * b), per component
 *   normal       N_t
 * The sums of decoded vertex d -- Theta_d, A_d, L_d (three components), S_d (three components) -- start from +0 and add the terms
 * of d's slots in ascending s, one after the other.  A vertex with more than 32 slots (n of them) instead sums 256 consecutive
 * ranges of ceil(n / 256) slots each in that way, each from +0, and adds the 256 partial sums in range order, as the normals and
 * creases do: an association n alone determines.
 * The class of d, from e: 0 isolated, d has no slot at all; 3 irregular, d is a decoded end (vs of either end of the first side) of
 * an edge with more than two sides; 2 boundary, d is a decoded end of an edge with exactly one side and is not irregular; 1 interior,
 * everything else.  8 is or-ed in where A_d is not usable, that is where A_d > 0 and finite fails -- which includes every isolated
 * vertex: it reads 8.
 * Buffers by name, U rows each; row u holds the value of decoded vertex vs[u], as "normals" does:
 *   "vertex_class"  u32 [U]     as above
 *   "vertex_area"   f32 [U]     (float)A_d; +0 where A_d is not usable
 *   "angle_defect"  f32 [U]     (float)(tau - Theta_d), tau the double nearest 2 pi for classes 1 and 3 and the double nearest pi for
 *                               class 2 (bit 8 aside); +0 for class 0
 *   "gaussian"      f32 [U]     (float)((tau - Theta_d) / A_d); +0 where A_d is not usable
 *   "mean_normal"   f32 [U, 3]  (float)(L_d / (4.0 * A_d)) per component, the product first: the mean curvature vector H n.  Zeros
 *                               where A_d is not usable
 *   "mean"          f32 [U]     (float)H_d, H_d = (L_d . S_d) / (|S_d| * (4.0 * A_d)): positive where the surface is convex towards
 *                               its area-weighted normal.  Where |S_d| is 0 or not finite, H_d = |L_d| / (4.0 * A_d).  +0 where A_d
 *                               is not usable
 * Totals: the term row of d is (A_d, tau - Theta_d, H_d * A_d), or (+0, +0, +0) where d is of class 0 or has bit 8.  The rows are
 * reduced in rounds, per column: a round replaces the rows by the sums of their consecutive chunks of 256 rows -- chunk c is the rows
 * [256 c, 256 c + 256), its sum starts from +0 and adds them in ascending order -- and rounds follow, at least one, until one row
 * is left.  D = 0: the totals are +0.
 * Determinism: the bits of every buffer and of the totals depend on r and e alone -- not on the run, on residency, or on the order
 * atomics complete in.
 * Refusals: null arguments, any flag bit, an r or e that does not fit m or each other (U / T / nf / E) or that lives on another
 * device: HRY_E_ARG; 3 T > 2^31, or a position list the normals' rule refuses: HRY_E_UNSUPPORTED; *out stays NULL and ctx stays
 * usable.
 * Out of scope: principal directions, curvature of polygon faces other than through their fan triangles, meshes on several devices.
 *   hry_curvature_count    U, the rows
 *   hry_curvature_get / _copy / _stat  as hry_creases_get / _copy / _stat
 *   hry_curvature_summary  out = { D, interior, boundary, irregular, isolated (classes by their low three bits), vertices with bit
 *                          8 }, counted over decoded vertices: device reductions during the build, no buffer is downloaded for them
 *   hry_curvature_totals   out = { sum of A_d, sum of (tau - Theta_d), sum of H_d * A_d } as above.  The second divided by 2 pi is,
 *                          on a closed manifold mesh, its Euler characteristic */
typedef struct hry_curvature hry_curvature;
#define HRY_VERTEX_ISOLATED   0u
#define HRY_VERTEX_INTERIOR   1u
#define HRY_VERTEX_BOUNDARY   2u
#define HRY_VERTEX_IRREGULAR  3u
#define HRY_VERTEX_DEGENERATE 8u   /* or-ed in: the vertex has no usable area */
int hry_curvature_build(hry_ctx *ctx, const hry_mesh *m, const hry_render *r, const hry_edges *e, uint32_t flags, hry_curvature **out);
uint64_t hry_curvature_count(const hry_curvature *c);             /* U: the rows, output vertices of r */
int hry_curvature_get(const hry_curvature *c, const char *name, const void **dev, uint64_t *rows, int *width, int *type);
int hry_curvature_copy(hry_ctx *ctx, const hry_curvature *c, const char *name, void *dst, int dst_is_device);
int hry_curvature_summary(const hry_curvature *c, uint64_t out[6]);
int hry_curvature_totals(const hry_curvature *c, double out[3]);
int hry_curvature_stat(const hry_curvature *c, double *device_ms, uint64_t *uploaded_bytes);
void hry_curvature_free(hry_curvature *c);

/* ---- ray queries on a render build: a bounding-volume hierarchy and a closest-hit cast ----------------------------------------------
 * hry_bvh_build builds, on ctx's device, a linear bounding-volume hierarchy over the triangles of r, a render build of m, and
 * hry_bvh_cast answers where rays first meet them.  The build reads r's "indices" and the float rows of its position list where they
 * lie in HBM: nothing is uploaded (uploaded_bytes is 0), the handle owns one allocation like the other results and keeps its own copy
 * of the positions it needs, so r may be freed afterwards.  flags must be 0.  The contract defines the result, not the way to it:
 * every bit of every buffer depends on r alone, every bit of a cast on the hierarchy and the rays alone, and a program that tests
 * every triangle against every ray by the rules below gets the same bits.
 * Let T be the triangles of r and I = indices; P[u] as in the edges' contract (the same position list, the same HRY_E_UNSUPPORTED
 * refusals).  "Least" and "greatest" of floats are taken in the floats' order with -0 below +0 (a total order: the result is one of
 * the values, whatever the order of the comparisons).
 * Live triangles: t is live when all nine floats of P[I[t][0]], P[I[t][1]], P[I[t][2]] are finite.  A dead triangle is in no leaf
 *   and is never hit.  L: the live triangles.
 * Boxes: the leaf box of t is, per axis, the least and the greatest of its three floats -- exact, no padding.  The scene box lo, hi
 *   is the least and the greatest over the live triangles' leaf boxes.
 * Code: in double, c_k = ((P0_k + P1_k) + P2_k) / 3.0; cell_k = 0 where hi_k == lo_k, otherwise ((c_k - lo_k) / (hi_k - lo_k)) *
 *   1024.0 truncated toward zero and clamped to 0 .. 1023.  The 30-bit code interleaves the cells: bit 3 j + 2 is x's bit j, bit
 *   3 j + 1 y's, bit 3 j z's.
 * Leaves: the live triangles in ascending (code, t).  Leaf i has the key code_i * 2^32 + i; the keys are distinct.
 * Tree: the binary radix tree of the keys, L - 1 internal nodes in Karras's numbering.  The root is internal node 0 and covers the
 *   leaves [0, L - 1].  A node that covers [a, b] splits behind gamma, the largest j in [a, b) whose key shares more leading bits with
 *   key_a than key_a shares with key_b.  Its left child covers [a, gamma]: leaf gamma where a == gamma, otherwise internal node gamma;
 *   its right child covers [gamma + 1, b]: leaf gamma + 1 where gamma + 1 == b, otherwise internal node gamma + 1.  A child word has
 *   bit 31 set for a leaf.  L = 1: no internal node, the leaf is the tree.  L = 0: everything is empty.
 *   Every level consumes at least one of a key's 62 significant bits, so no leaf has more than 62 internal nodes above it.
 * Node boxes: per axis the least / greatest of the two children's boxes.
 * Buffers by name:
 *   "leaf_tri"        u32 [L]         the triangle of leaf i
 *   "leaf_code"       u32 [L]         its code
 *   "leaf_box"        f32 [L, 6]      min x y z, max x y z
 *   "leaf_positions"  f32 [L, 9]      its three positions (the cast reads these, not r)
 *   "node_children"   u32 [L - 1, 2]  left, right
 *   "node_box"        f32 [L - 1, 6]
 *   "scene_box"       f32 [1, 6]      (+inf x 3, -inf x 3) where L = 0
 * Refusals: null arguments, any flag bit, an r that does not fit m (U / T / nf) or that lives on another device: HRY_E_ARG;
 * 3 T > 2^31, or a position list the normals' rule refuses: HRY_E_UNSUPPORTED; *out stays NULL and ctx stays usable.
 *   hry_bvh_count    L, the leaves
 *   hry_bvh_get / _copy / _stat  as hry_curvature_get / _copy / _stat
 *   hry_bvh_summary  out = { T, L, T - L, distinct codes, depth, 0 }; depth: the largest number of internal nodes between the root
 *                    and a leaf, both ends counted, 0 for L <= 1 and at most 62.  Device reductions during the build
 *
 * hry_bvh_cast: ray i reads three floats at origins + i * origin_stride bytes and three at dirs + i * dir_stride bytes; the strides
 * are multiples of 4, and a stride of 0 means one value for all rays.  The outputs are dense: hit_tri [n_rays], hit_t [n_rays],
 * hit_uv [n_rays, 2]; hit_t, hit_uv, stat and device_ms may be NULL.  Without flags the five pointers are memory of ctx's device,
 * checked as hry_mesh_from_device checks its columns, read and written on hry_ctx_stream, and the call returns when the results are
 * written; with HRY_CAST_HOST all five are host memory, staged by the library.
 * All arithmetic is in double on the widened floats, every operation individually rounded in the written order; a . b =
 * (a.x b.x + a.y b.y) + a.z b.z, a x b as in the normals' contract.  O, D: the ray's origin and direction.
 * Valid ray: O and D finite and D != (0, 0, 0).  Any other ray misses.
 * Interval of a box [lo, hi] for a valid ray -- the one rule, for leaf and node boxes alike.  An axis with D_k == 0 (-0 included):
 *   the box fails where O_k < lo_k or O_k > hi_k, otherwise the axis sets no bound.  Another axis: inv = 1.0 / D_k, a = (lo_k - O_k) *
 *   inv, c = (hi_k - O_k) * inv, n_k = min(a, c), f_k = max(a, c).  n is the largest n_k, f the least f_k; n' = n - |n| * 2^-30,
 *   f' = f + |f| * 2^-30; near = max(tmin, n'), far = min(tmax, f').  The box passes when near <= far.  Everything here is finite
 *   but tmin and tmax: no NaN arises.  Every step is monotone in lo downwards and in hi upwards, rounding included, so a box that
 *   contains another has a near no greater and a far no smaller than the inner box's, exactly: a subtree whose box fails holds no
 *   leaf whose box passes (DESIGN.md "Bvh").
 * Hit of leaf triangle t: its own leaf box must pass, with the interval [near_t, far_t].  Then e1 = P1 - P0, e2 = P2 - P0, p = D x e2,
 *   det = e1 . p, s = O - P0, q = s x e1, u = (s . p) / det, v = (D . q) / det, tt = (e2 . q) / det; t is accepted when det is finite
 *   and not 0 (both facings count), u >= 0, v >= 0, u + v <= 1 and near_t <= tt <= far_t.  A NaN fails every comparison.
 * Answer: the accepted triangle with the least tt, ties to the least triangle number: hit_tri = t, hit_t = (float)tt, hit_uv =
 *   ((float)u, (float)v).  A miss gives HRY_NO_ELEMENT, +inf, (0, 0).
 * Not promised: watertightness.  A ray through a shared edge or vertex may miss both triangles: u, v and u + v are rounded per
 *   triangle.  (The widened boxes only keep the box clause from deciding such a ray; they do not close the gap.)
 * stat = { rays that hit, box intervals evaluated }; the second depends on the walk (it is what a hierarchy saves over L tests a
 *   ray) and is no part of the bit contract.  device_ms: the kernel.
 * tmin > tmax is no error: every ray misses.  n_rays = 0 succeeds and touches nothing.
 * Refusals (HRY_E_ARG): a null ctx or b; null hit_tri, origins or dirs with n_rays > 0; unknown flags; a stride that is not a
 * multiple of 4; NaN tmin or tmax; a pointer that is not what the flags say, is misaligned, or whose rows extend past its allocation;
 * a b on another device than ctx's. */
typedef struct hry_bvh hry_bvh;
#define HRY_CAST_HOST 1u   /* origins, dirs, hit_tri, hit_t and hit_uv are host memory */
int hry_bvh_build(hry_ctx *ctx, const hry_mesh *m, const hry_render *r, uint32_t flags, hry_bvh **out);
uint64_t hry_bvh_count(const hry_bvh *b);             /* L: the leaves, live triangles of r */
int hry_bvh_get(const hry_bvh *b, const char *name, const void **dev, uint64_t *rows, int *width, int *type);
int hry_bvh_copy(hry_ctx *ctx, const hry_bvh *b, const char *name, void *dst, int dst_is_device);
int hry_bvh_summary(const hry_bvh *b, uint64_t out[6]);
int hry_bvh_stat(const hry_bvh *b, double *device_ms, uint64_t *uploaded_bytes);
void hry_bvh_free(hry_bvh *b);
int hry_bvh_cast(hry_ctx *ctx, const hry_bvh *b, uint64_t n_rays, const float *origins, uint64_t origin_stride, const float *dirs, uint64_t dir_stride,
                 double tmin, double tmax, uint32_t flags, uint32_t *hit_tri, float *hit_t, float *hit_uv, uint64_t stat[2], double *device_ms);

/* hry_bvh_nearest answers, for every query point, which triangle of the hierarchy lies closest within max_dist, how far and where
 * on it.  Point i reads three floats at points + i * point_stride bytes; the stride is a multiple of 4, and 0 means one point for
 * all.  The outputs are dense: near_tri [n_points], near_d2 [n_points] doubles, near_uv [n_points, 2], near_point [n_points, 3];
 * near_d2, near_uv, near_point, stat and device_ms may be NULL.  The contract defines the result, not the way to it: every bit
 * depends on the hierarchy and the points alone, and a program that tests every point against every leaf by the rules below gets
 * the same bits.  All arithmetic is in double on the widened floats, every operation individually rounded in the written order;
 * a . b and a x b as in the cast's contract.  Q: the point.
 * Valid point: Q has three finite floats.  Any other point is unanswered.
 * Radius: r2 = max_dist * max_dist.  A negative max_dist is no error: every point is unanswered.  +inf is allowed; NaN is refused.
 * Bound of a box [lo, hi] -- the one rule, for leaf and node boxes alike: g_k = max(max(lo_k - Q_k, Q_k - hi_k), 0), b2 =
 *   (g_x g_x + g_y g_y) + g_z g_z.  Every step is monotone in lo downwards and in hi upwards, rounding included, so a box that
 *   contains another has a bound no greater, exactly.
 * Segment (A, B): d = B - A, l = d . d, s = 0 where l == 0, otherwise ((Q - A) . d) / l clamped to [0, 1] (a value below 0 becomes
 *   0, one above 1 becomes 1, any other stays).
 * Candidates of leaf triangle t, with e1 = P1 - P0, e2 = P2 - P0 and s = Q - P0, in this order:
 *   (a) the face: n = e1 x e2, nn = n . n; where nn > 0, u = ((s x e2) . n) / nn and v = ((e1 x s) . n) / nn, and the face is a
 *       candidate when u >= 0, v >= 0 and u + v <= 1;
 *   (b) segment (P0, P1) with (u, v) = (s, 0);  (c) segment (P1, P2) with (u, v) = (1 - s, s);  (d) segment (P2, P0) with (u, v) =
 *       (0, 1 - s).
 *   For each candidate C = P0 + (u e1 + v e2), per component, and d2 = (Q - C) . (Q - C).  The triangle takes the first candidate
 *   with the least d2: a later candidate replaces an earlier one only when strictly less.  A NaN fails every comparison.  A
 *   triangle without area answers as the segment or the point it is.
 * The triangle's distance: d2_t = max(that d2, the bound of t's own leaf box).  Mathematically the bound never exceeds the
 *   distance; the rounding of C can break that by an ulp, and with the clamp d2_t >= bound(leaf box) >= bound(every box above it)
 *   holds exactly: a subtree whose bound is strictly greater than the best d2_t so far holds nothing better (an equal bound may
 *   hold a lower triangle number; DESIGN.md "Bvh").
 * Answer: among the triangles with d2_t <= r2 the one with the least d2_t, ties to the least triangle number: near_tri = t,
 *   near_d2 = d2_t (the squared distance, as a double: the quantity compared; no square root enters the bit contract), near_uv =
 *   ((float)u, (float)v), near_point = (float) of C's components.  An unanswered point gives HRY_NO_ELEMENT, +inf, (0, 0) and
 *   (0, 0, 0).
 * stat = { points answered, box bounds evaluated, the bits of the largest near_d2 among the answered points (0 where none was) }.
 *   The third is an integer maximum of the doubles' words -- non-negative doubles order as their words, so the order decides
 *   nothing; there are no floating-point atomics.  The second depends on the walk and is no part of the bit contract.
 *   device_ms: the kernel.
 * Pointers, staging and refusals as for hry_bvh_cast: without flags points and the four outputs are memory of ctx's device, with
 *   HRY_NEAREST_HOST host memory staged by the library; near_d2 must be 8-byte aligned, the others 4-byte.  n_points = 0 succeeds
 *   and touches nothing.  Refusals (HRY_E_ARG): a null ctx or b; null near_tri or points with n_points > 0; unknown flags; a stride
 *   that is not a multiple of 4; NaN max_dist; a pointer that is not what the flags say, is misaligned, or whose rows extend past
 *   its allocation; a b on another device than ctx's.  A refusal writes nothing and leaves ctx usable. */
#define HRY_NEAREST_HOST 1u   /* points, near_tri, near_d2, near_uv and near_point are host memory */
int hry_bvh_nearest(hry_ctx *ctx, const hry_bvh *b, uint64_t n_points, const float *points, uint64_t point_stride,
                    double max_dist, uint32_t flags,
                    uint32_t *near_tri, double *near_d2, float *near_uv, float *near_point,
                    uint64_t stat[3], double *device_ms);

/* hry_intersections_build answers whether the surface passes through itself: the pairs of the hierarchy's triangles of which an
 * edge of one meets the other.  It reads the hierarchy alone -- "leaf_tri", "leaf_box", "leaf_positions", "node_children",
 * "node_box" --, so the mesh and the render build may have been freed.  The contract defines the result, not the way to it: every
 * bit of the buffers depends on the hierarchy alone, and a program that tests every pair of leaves by the rules below gets the same
 * bits.  All arithmetic is in double on the widened floats, every operation individually rounded in the written order; a . b and
 * a x b as in the cast's contract.
 * Proper triangle: a leaf triangle with n = (P1 - P0) x (P2 - P0) and n . n > 0, as the face candidate of hry_bvh_nearest asks.
 *   Dead triangles are no leaves and are in no pair; an improper triangle (a segment, a point) is tested against nothing.
 * Shared corners: two corners are the same when their three floats compare equal with == (so -0 equals +0): by position, not by
 *   index -- an unwelded render build's neighbours share positions, not numbers.  share(t, s): the corners of t that are the same
 *   as some corner of s; the corners of a proper triangle are distinct, so it is 0 .. 3 and share(t, s) = share(s, t).
 * Segment against triangle: meets(A, B, tri) is the hit of hry_bvh_cast with O = A, D = B - A -- e1, e2, p, det, s, q, u, v, tt
 *   as there --, true when det is finite and not 0, u >= 0, v >= 0, u + v <= 1 and 0 <= tt <= 1.  A NaN fails every comparison.
 *   Edge k of a triangle is (P_k, P_(k + 1) % 3), in that direction.
 * The unordered pair {t, s}, t < s, intersects when all of these hold:
 *   1. their leaf boxes overlap, closed, on the floats: lo_t <= hi_s and lo_s <= hi_t on the three axes;
 *   2. both are proper and share(t, s) <= 1;
 *   3. an admitted edge of one meets the other.  With share = 0 all six edges are admitted; with share = 1 only the edge opposite
 *      the shared corner, on either side: two tests (the edges through the shared corner touch the other triangle there and
 *      nowhere else, unless the triangles are coplanar).  The OR of the tests does not depend on their order, and no test on
 *      which triangle is called the first.
 * What follows, and is no defect:
 *   touching counts -- a corner on a face, an edge against an edge;
 *   coplanar overlaps are not found: det = 0 fails every test;
 *   pairs that share an edge or all three corners are never tested: a fold about a shared edge is what "edge_cos" of
 *   hry_edges_build tells;
 *   near-coplanar pairs are decided by the rounding -- deterministically, like everything else here.
 * Buffers by name:
 *   "pairs"        u32 [P, 2]  (t, s), t < s, triangle numbers of the render build, ascending lexicographically
 *   "pair_shared"  u32 [P]     share(t, s): 0 or 1
 *   "tri_pairs"    u32 [T]     in how many pairs triangle t is (a dead or improper one: 0)
 *   hry_intersections_count    P
 *   hry_intersections_get / _copy / _stat / _free  as hry_bvh_get / _copy / _stat / _free
 *   hry_intersections_summary  out = { T, C, N, P, H, box tests }; C: the pairs of leaves t < s whose boxes overlap, improper and
 *                    edge-sharing ones included; N: those of them with both proper and share <= 1, the pairs that reach meets; H:
 *                    the triangles with tri_pairs > 0.  The sixth word, the box tests the walk made, is the one word that depends
 *                    on the walk (it is what a hierarchy saves over L tests a leaf) and is no part of the bit contract.  Integer
 *                    device reductions; there are no floating-point atomics.
 * Refusals: null arguments ("null argument", before any device is touched), any flag bit, a b on another device than ctx's:
 * HRY_E_ARG; P >= 2^31: HRY_E_UNSUPPORTED; *out stays NULL and ctx stays usable. */
typedef struct hry_intersections hry_intersections;   /* a result handle like hry_bvh */
int hry_intersections_build(hry_ctx *ctx, const hry_bvh *b, uint32_t flags, hry_intersections **out);   /* flags: none */
uint64_t hry_intersections_count(const hry_intersections *i);   /* P: the pairs */
int hry_intersections_get(const hry_intersections *i, const char *name, const void **dev, uint64_t *rows, int *width, int *type);
int hry_intersections_copy(hry_ctx *ctx, const hry_intersections *i, const char *name, void *dst, int dst_is_device);
int hry_intersections_summary(const hry_intersections *i, uint64_t out[6]);
int hry_intersections_stat(const hry_intersections *i, double *device_ms, uint64_t *uploaded_bytes);
void hry_intersections_free(hry_intersections *i);

/* hry_mesh_flip_faces returns a clone of m in which every face f with face_flip[f] != 0 (nf host words, for instance "face_flip" of
 * hry_orient_build), (v0, v1, ..., vk-1), has become (v0, vk-1, ..., v1).  Every per-corner array follows its corner: the origins,
 * and with general bindings the corners' record rows.  The clone's half-edge twins are matched afresh when first needed; it has no
 * device, render or order token.  Applying it twice with the same flags gives the original arrays.  A partial mesh or a null
 * argument: HRY_E_ARG, *out stays NULL */
int hry_mesh_flip_faces(const hry_mesh *m, const uint32_t *face_flip, hry_mesh **out);

/* ---- meshes from device buffers --------------------------------------------------------------------------------------
 * hry_mesh_from_device is hry_mesh_from_arrays for data that already lives on ctx's device (the other direction of
 * hry_render_build).  A component is a strided column: row i's value of `type` at (const uint8_t*)data + i * stride, where data is
 * device memory of ctx's device aligned to the type's size and stride a non-zero multiple of it.  `name` and `type` mean what
 * v_names / v_types of hry_mesh_from_arrays mean.  d_degrees: nf uint8 (NULL: every face a triangle); d_indices: n_indices entries
 * of index_type (HRY_UINT or HRY_LONG), faces in order, corners in order; fcols: f_ncomp columns of nf rows (the face list).
 *   Equal to the host constructor: without HRY_INGEST_WELD the mesh is the one hry_mesh_from_arrays builds from the same values --
 *     lists, component order, names and types, degrees, half-edge order (org is the flattened index list).  Twins are matched on the
 *     device by the code hry_mesh_upload uses (hubs on the host, as there), so they equal what an upload computes.
 *   Residency: on return ctx holds the records, org, twins and face offsets in HBM; the mesh and ctx share one token exactly as after
 *     hry_mesh_upload (the earlier resident mesh of ctx is displaced), so hry_bounds / hry_requant / hry_encode on ctx upload nothing
 *     for it.  The host copies (connectivity and records) are filled too: the result is an ordinary PLY-layout mesh.
 *   Input buffers: read on ctx's stream (hry_ctx_stream) and not kept; the caller has finished writing them before the call.
 *   Refusals, with the host path's code and text where it has one: an index out of range (a negative HRY_LONG too): HRY_E_ARG,
 *     "vertex index out of range"; a degree outside 3..255, more than 32 components in a list, more than 2^32 - 1 half-edges:
 *     HRY_E_UNSUPPORTED; sum(degrees) != n_indices, a pointer that is not device memory of ctx's device, a misaligned column, a
 *     zero stride, a bad type or index_type: HRY_E_ARG.  *out stays NULL and ctx stays usable.  The checks run on the device into
 *     one status word (vector atomics) that is read back once; nothing is written out of bounds on the way.
 *   HRY_INGEST_WELD merges vertices whose records are equal byte for byte: the key of a row is every component as stored (-0.0 and
 *     +0.0 stay apart, identical NaN bit patterns merge).  Output vertices are numbered in order of first occurrence over input rows
 *     0 .. nv - 1, deterministically.  Face indices go through the map; faces, face records and corners are kept as they are (an
 *     unreferenced row stays a vertex, a face that collapses keeps its corners).  d_remap (NULL, or nv u32 of device memory) receives
 *     the output vertex of every input row; hry_mesh_nv is the welded count.  The result equals hry_mesh_from_arrays of the welded
 *     arrays.  Welding with v_ncomp == 0 is HRY_E_ARG.
 * The result always has the PLY layout; general bindings (OBJ regions, corner lists) are hry_mesh_from_device_corners' below. */
typedef struct hry_dev_column {
    const void *data;     /* device memory of ctx's device, aligned to the type's size */
    uint64_t stride;      /* bytes between rows: a non-zero multiple of the type's size */
    const char *name;     /* PLY component name ("x", "nx", "red", ...), interpreted as hry_mesh_from_arrays does */
    int32_t type;         /* HRY_FLOAT .. HRY_CHAR: the stored type */
} hry_dev_column;
#define HRY_INGEST_WELD 1
int hry_mesh_from_device(hry_ctx *ctx, uint32_t nv, const hry_dev_column *vcols, int v_ncomp,
                         uint32_t nf, const uint8_t *d_degrees, const void *d_indices, int index_type, uint64_t n_indices,
                         const hry_dev_column *fcols, int f_ncomp, int flags, uint32_t *d_remap, hry_mesh **out);

/* hry_mesh_from_device_corners is hry_mesh_from_obj for data that already lives on ctx's device: positions per vertex, texture
 * coordinates and normals per corner with index buffers of their own, a material per face (the other direction of hry_render_build
 * for meshes with general bindings).  pos / tex / nrm: the rows of one list as float columns (hry_dev_column as above; type must be
 * HRY_FLOAT, name is not read) and, per corner, the row it names: `indices` holds n_indices entries of index_type (HRY_UINT or
 * HRY_LONG), faces in order, corners in order.  tex and nrm may be NULL.  d_degrees: nf uint8 (NULL: every face a triangle);
 * d_face_material: nf uint16 (NULL: one region).
 *   Result: a mesh with general bindings of exactly the shape hry_mesh_from_obj creates.  List 0: the positions, vertex target,
 *     pos->ncomp one of 3, 4, 6, 7, 8 with the reader's interpretations (POS; COLOR from component 3 on when ncomp > 4).  Then tex,
 *     if given (corner target, TEX, ncomp 2 or 3), then nrm, if given (corner target, NORMAL, ncomp 3).  All components HRY_FLOAT,
 *     unquantised.  One vertex region binding list 0, vertex v naming record v.  Slots per face / vertex / corner: 0 / 1 / 2, as the
 *     reader sets them.  Every face region binds the corner lists given, compacted: slot 0 is tex and the next nrm, normals alone sit
 *     in slot 0; an unused slot of a corner holds 0.  org[c] = pos->indices[c]; slot s of corner c holds the corner's row in that
 *     slot's list.  Degrees, face offsets and half-edge order as hry_mesh_from_device.
 *   Face regions: the distinct values of d_face_material, numbered in order of first occurrence over faces 0 .. nf - 1 (what the
 *     reader does with "usemtl" when every face carries the same kinds of index).  More than 128: HRY_E_UNSUPPORTED.
 *   Equal to the reader: without HRY_INGEST_WELD the mesh is the one hry_mesh_from_obj builds from the plain text of the same arrays
 *     ("v" / "vt" / "vn" lines in row order, "f a/b/c" lines, "usemtl" where the material changes), array for array; twins are matched
 *     on the device by the code hry_mesh_upload uses, so they equal what an upload computes.
 *   HRY_INGEST_WELD welds every list given on its own: rows equal byte for byte merge (-0.0 and +0.0 stay apart, identical NaN bit
 *     patterns merge), output records are numbered in order of first occurrence over the list's rows, the corners' indices go through
 *     the list's map; unreferenced rows stay records (of positions: vertices), faces are kept as they are.  The result equals the
 *     unwelded constructor applied to the welded arrays.  With all three `indices` equal this inverts hry_render_build's unweld:
 *     indices into one table of (position, uv, normal) rows become one connectivity plus shared corner records.
 *   d_remap: NULL, or three pointers (0 pos, 1 tex, 2 nrm; each NULL or `rows` u32 of device memory) that receive the output record
 *     of every input row (the identity without HRY_INGEST_WELD).
 *   Residency: on return ctx holds what hry_mesh_upload would have put there for this mesh -- the records of every list, org, twins,
 *     face offsets and the binding tables -- under one token shared with the mesh, so hry_mesh_resident is 1 and hry_bounds /
 *     hry_requant / hry_encode on ctx upload nothing for it, in both profiles.  The host copies are filled too.  Input buffers are
 *     read on ctx's stream and not kept.
 *   Refusals (*out stays NULL, ctx stays usable; its earlier resident mesh may be displaced): a row index out of range, a negative
 *     HRY_LONG too: HRY_E_ARG, "vertex index out of range" / "texture index out of range" / "normal index out of range" by the
 *     list; sum(degrees) != n_indices, a pointer that is not device memory of ctx's device, a misaligned or zero-stride column, a
 *     column type other than HRY_FLOAT, an ncomp outside the sets above, pos == NULL, a bad index_type, unknown flags: HRY_E_ARG; a
 *     degree outside 3..255, more than 2^32 - 1 half-edges: HRY_E_UNSUPPORTED.  The checks run on the device into one status word
 *     that is read back once, with the welded counts and the number of regions; nothing is written out of bounds on the way.
 * Out of scope: several vertex lists or regions (the reader's "v" lines of different widths), face lists, components that are not
 * floats, faces that differ in the kinds of index they carry. */
typedef struct hry_dev_rows {
    const hry_dev_column *cols;   /* ncomp columns; type must be HRY_FLOAT; name is not read (may be NULL) */
    int32_t ncomp;
    uint32_t rows;
    const void *indices;          /* n_indices entries of index_type, faces in order, corners in order */
} hry_dev_rows;                   /* 24 bytes */
int hry_mesh_from_device_corners(hry_ctx *ctx, const hry_dev_rows *pos, const hry_dev_rows *tex /* or NULL */,
                                 const hry_dev_rows *nrm /* or NULL */, uint32_t nf, const uint8_t *d_degrees,
                                 int index_type, uint64_t n_indices, const uint16_t *d_face_material /* or NULL */,
                                 int flags, uint32_t *const d_remap[3] /* or NULL; entries may be NULL */, hry_mesh **out);
/* 1: ctx holds m's records and connectivity in HBM (hry_mesh_from_device[_corners] or hry_mesh_upload, nothing on ctx since that displaced
 * them), so hry_bounds / hry_requant / hry_encode on ctx upload nothing for m */
int hry_mesh_resident(const hry_ctx *ctx, const hry_mesh *m);

/* ---- numbering maps of an encode: source order <-> decoded order -----------------------------------------------------
 * The decoder numbers vertices, faces and half-edges in traversal order (cbm/decoder.h:48,75,145,162), and with general bindings
 * the records of every list in creation order: hry_decode(hry_encode(m)) is m up to a permutation of vertices, of faces, of every
 * list's records, and a rotation of every face.  hry_encode with HRY_FLAG_ORDER keeps those permutations on ctx's device, and
 * hry_order_take hands them out as a handle that owns its memory.  Maps by name, each u32 in HBM:
 *   "vertex"    [nv]  decoded vertex of every source vertex
 *   "face"      [nf]  decoded face of every source face
 *   "corner"    [ne]  decoded half-edge of every source half-edge
 *   "list<l>"   [records of list l]  general bindings only (l in decimal): decoded record of every source record.  In the PLY layout
 *                     list 1 is "vertex" and list 0 is "face", and the "list" names are absent
 *   "<name>_inv"      the inverse: its rows are the decoded mesh's elements as its header declares them, its values source elements
 * Contract, with D = hry_decode(hry_encode(m)) in either profile and m's twins as hry_encode left them:
 *   D.org[corner[c]] == vertex[m.org[c]] and D.twin[corner[c]] == corner[m.twin[c]] for every half-edge c; the corners of source
 *   face f are the corners of decoded face face[f], same degree, same cyclic order, another start; the record bytes of D at
 *   vertex[v] / face[f] / list<l>[r] are m's at v / f / r (m holds the quantised values already); every binding table of D at a
 *   mapped element holds the mapped record; D's face region at face[f] is m's at f.
 * A vertex no face names and a record no element names are never coded: they map to HRY_NO_ELEMENT, and so do the decoded mesh's
 * filler rows in the inverse.  Everywhere else the maps are bijections: x_inv[x[i]] == i.  Both profiles give the same maps, and
 * the flag changes neither the container's bytes nor the mesh's twins.
 *   hry_order_take   valid when the last call on ctx was a successful hry_encode of m with HRY_FLAG_ORDER; anything else -- no flag,
 *                    another call on ctx in between, a second take -- is HRY_E_ARG.  The handle's one device allocation stays valid
 *                    whatever the context does later; free it before the context.
 *   hry_order_get    a map by name: device address and rows (rows 0: absent)
 *   hry_order_copy   the whole map to dst (device or host memory) on ctx's stream; returns when it is there
 *   hry_order_apply  moves rows of row_bytes bytes through the map `kind` ("vertex", "face", "corner", "list<l>") on ctx's stream and
 *                    returns when it is done.  HRY_ORDER_TO_DECODED: dst row j = src row kind_inv[j]; HRY_ORDER_TO_SOURCE: dst row
 *                    i = src row kind[i]; a row whose map entry is HRY_NO_ELEMENT becomes zero bytes.  Row r of a buffer starts
 *                    r * stride bytes behind its pointer; only the row_bytes of each dst row are written.  dst_rows must be the row
 *                    count of the map that indexes dst, and src holds as many rows.  A stride below row_bytes, row_bytes 0, a null
 *                    pointer, a pointer that is not memory of ctx's device, overlapping src and dst ranges, an unknown kind or
 *                    direction: HRY_E_ARG, and ctx stays usable.
 * HRY_FLAG_ORDER on a shard (a mesh that carries runs) and in hry_encode_sharded is HRY_E_UNSUPPORTED. */
#define HRY_FLAG_ORDER 16            /* hry_encode: keep the numbering maps of this encode for hry_order_take */
#define HRY_NO_ELEMENT 0xFFFFFFFFu
typedef struct hry_order hry_order;
int  hry_order_take(hry_ctx *ctx, const hry_mesh *m, hry_order **out);
int  hry_order_get(const hry_order *o, const char *name, const void **dev, uint64_t *rows);   /* u32 [rows] in HBM; rows 0: absent */
int  hry_order_copy(hry_ctx *ctx, const hry_order *o, const char *name, void *dst, int dst_is_device);
#define HRY_ORDER_TO_DECODED 0
#define HRY_ORDER_TO_SOURCE  1
int  hry_order_apply(hry_ctx *ctx, const hry_order *o, const char *kind, int direction,
                     const void *d_src, uint64_t src_stride, void *d_dst, uint64_t dst_stride,
                     uint64_t row_bytes, uint64_t dst_rows);
void hry_order_free(hry_order *o);

/* ---- what a quantisation cost: per-component error of one mesh against another, on the device -------------------------
 * hry_distortion_build compares mesh a (the source) with mesh b -- typically hry_decode(hry_encode(m)) for a clone m of a after
 * hry_requant -- component by component, through the numbering map of the encode that relates them, and keeps the statistics
 * (and, with HRY_DISTORTION_ROWS, one error value per row in HBM: a heat map next to hry_render_build's buffers).
 *   Meshes: the same number of lists (more than 16: HRY_E_UNSUPPORTED), the same layout (PLY or general bindings), and per list
 *     the same target, component count (more than 32: HRY_E_UNSUPPORTED) and ORIGINAL component types: HRY_E_ARG otherwise.  The
 *     quantisation bits may differ on either side.  A quantised list without bounds and a partial mesh are HRY_E_ARG, as in
 *     hry_render_build.  Lists without components or without a target are not compared; in the PLY layout lists 0 and 1 are.
 *   Rows: row i of list l of a is paired with row map_l[i] of b.  o == NULL: the identity, and the lists' counts must be equal
 *     (HRY_E_ARG).  With o: "vertex" for list 1 and "face" for list 0 in the PLY layout, "list<l>" with general bindings; the
 *     map's rows must equal a's count, and every entry other than HRY_NO_ELEMENT must be below b's count: HRY_E_ARG, "order does
 *     not fit the meshes".  The entries are checked on the device into one status word (vector atomics) that is read back once;
 *     nothing is read out of bounds on the way.  A row whose entry is HRY_NO_ELEMENT counts in `skipped`.
 *   Value: x (of a) and y (of b) are what hry_requant(..., clear = 1) gives for the component in its original type (the reference's
 *     -c; unquantised components as stored), converted to double: floats widen exactly, 64-bit integers round to nearest.
 *     e = y - x, one rounded double subtraction.  A pair is compared when x and y are both finite; otherwise it counts in
 *     `nonfinite` and enters no maximum, sum or range.
 *   max_abs, argmax (ties: the lowest row of a, whatever the grid), a_min and a_max are exact.  sum_sq adds the individually
 *     rounded e*e in a reduction tree that is fixed by the row count alone, without floating-point atomics: the same bits from
 *     run to run and whether the inputs were resident or uploaded.  The association itself is not part of the contract.
 *   Positions: the position list is list 1 in the PLY layout, with general bindings the lowest-numbered vertex-target list, when
 *     it has at least three POS components.  Over its first three: d2 = (ex*ex + ey*ey) + ez*ez, dist = sqrt(d2); a row is
 *     compared when all three pairs are finite; sum_sq_dist sums d2 under the same rule as sum_sq.
 *   HRY_DISTORTION_ROWS: for every compared list a buffer "error<l>", f32, one value per row of a:
 *     (float) sqrt(sum over the list's components, in component order, of e*e of the compared pairs); a skipped row holds 0.
 *   Unknown flag bits: HRY_E_ARG.
 *   Residency: when b is the mesh hry_decode just returned on ctx and nothing has touched ctx or b since (hry_render_build's
 *     test), b's records are read where the decode left them; when a is ctx's resident mesh (hry_mesh_resident), its records are
 *     read in place.  Whatever is not resident is uploaded (uploaded_bytes: the records that went up); the results are the same
 *     either way.  Neither the encoder's resident mesh nor the decode's buffers are disturbed: hry_render_build of b afterwards
 *     still finds them.  On any refusal *out stays NULL and ctx stays usable.
 *   The handle owns its one device allocation and the host copy of the statistics; free it before the context.
 *   hry_distortion_component  the record of component c of list l; an uncompared list, a bad l or c: HRY_E_ARG
 *   hry_distortion_position   the Euclidean displacement of the positions; list -1 (everything else 0): the meshes have none
 *   hry_distortion_position_component  where the position components begin in that list
 *   hry_distortion_get / _copy / _stat  as hry_render_get / _copy / _stat; device_ms: the two kernels, by events */
typedef struct hry_distortion hry_distortion;
#define HRY_DISTORTION_ROWS 1u      /* also build the per-row buffers "error<l>" */
int  hry_distortion_build(hry_ctx *ctx, const hry_mesh *a, const hry_mesh *b, const hry_order *o /* or NULL */,
                          uint32_t flags, hry_distortion **out);
typedef struct hry_comp_error {
    double   max_abs;      /* max |e| over the compared pairs; 0 when there is none */
    double   sum_sq;       /* sum of e*e over the compared pairs */
    double   a_min, a_max; /* range of a's finite values among the compared pairs (+inf / -inf when there is none) */
    uint64_t compared;     /* pairs with both values finite */
    uint64_t skipped;      /* rows of a whose map entry is HRY_NO_ELEMENT */
    uint64_t nonfinite;    /* mapped pairs with a NaN or infinity on either side */
    uint64_t changed;      /* compared pairs with e != 0, plus non-finite pairs whose two doubles differ in bits */
    uint32_t argmax;       /* lowest row of a that attains max_abs; HRY_NO_ELEMENT when compared == 0 */
    uint32_t reserved;
} hry_comp_error;          /* 72 bytes */
int  hry_distortion_component(const hry_distortion *d, int l, int c, hry_comp_error *out);
typedef struct hry_pos_error {
    double   max_dist, sum_sq_dist;
    uint64_t compared;
    uint32_t argmax;       /* lowest row attaining max_dist, HRY_NO_ELEMENT when compared == 0 */
    int32_t  list;         /* the position list, -1: the meshes have none (everything else 0) */
} hry_pos_error;
int  hry_distortion_position(const hry_distortion *d, hry_pos_error *out);
/* the first of the three position components within that list (they are consecutive), -1: the meshes have none -- what names the
 * hry_comp_error records whose a_min / a_max span the positions' bounding box */
int  hry_distortion_position_component(const hry_distortion *d);
int  hry_distortion_get(const hry_distortion *d, const char *name, const void **dev, uint64_t *rows);  /* "error<l>": f32 [rows] in HBM; rows 0: absent */
int  hry_distortion_copy(hry_ctx *ctx, const hry_distortion *d, const char *name, void *dst, int dst_is_device);
int  hry_distortion_stat(const hry_distortion *d, double *device_ms, uint64_t *uploaded_bytes);
void hry_distortion_free(hry_distortion *d);

/* ---- the shading error of a quantisation: the normal deviation per face -------------------------------
 * Quantised positions tilt small faces long before the displacement of a vertex is visible, and at low widths faces collapse to a
 * line or a point.  One quantity, reported after the fact by hry_distortion_build (HRY_DISTORTION_NORMALS) and before the fact, at
 * every width, by hry_quant_sweep_build_ex (HRY_SWEEP_NORMALS):
 *   Positions: P[v] = the first three POS components of the position list (hry_distortion_build's: list 1 in the PLY layout, the
 *     lowest-numbered vertex-target list with three POS components with general bindings), each taken as hry_distortion_build takes
 *     a value: what hry_requant(clear = 1) leaves in the original type, widened to double.
 *   Row of vertex v in the position list: v in the PLY layout; with general bindings the record v's region binds (one k_rows_of pass,
 *     as in hry_render_build) -- every vertex region must bind the list, otherwise the normals part is absent with
 *     hry_render_build_ex's reason, "normals: a vertex region that does not bind the position list".
 *   Face normal: face f has corners c_0 .. c_(d-1); N_f, a x b and |a| are those of hry_render_build_ex's normals contract: N_f = the
 *     sum over k = 1 .. d-2 of (P[c_k] - P[c_0]) x (P[c_(k+1)] - P[c_0]) in that order, a x b = (a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z,
 *     a.x*b.y - a.y*b.x), |a| = sqrt(a.x*a.x + a.y*a.y + a.z*a.z), every operation an individually rounded IEEE double operation in
 *     the written order; n = N / |N|, one division per component.
 *   Chord: N_x from the source's positions, N_y from the other side's; d = n_y - n_x per component, c2 = (d.x*d.x + d.y*d.y) + d.z*d.z,
 *     chord = sqrt(c2) = 2 sin(theta / 2) for the angle theta between the normals.  The chord, not the angle, is the device's
 *     quantity: it needs only + - * / sqrt (the same bits anywhere) and is monotone in the angle on [0, pi].
 *   Classes: every face falls in exactly one, tested in this order -- skipped: a corner's row maps to HRY_NO_ELEMENT (or lies outside
 *     the tables: nothing is read there); nonfinite: a corner position component is NaN or infinite on either side; degenerate: |N_x|
 *     is 0 or not finite (the source face has no normal); collapsed: |N_y| is 0 or not finite (the quantisation took the normal
 *     away); compared: everything else.  The five counters sum to the face count.
 *   max_chord, argmax and the counters are exact.  sum_sq_chord adds the individually rounded c2 in a tree fixed by the face count
 *     alone, without floating-point atomics: the same bits from run to run, resident or uploaded.
 * hry_chord_angle / hry_angle_chord, host only: 2 * asin(min(chord / 2, 1)) radians, and 2 * sin(radians / 2).  A negative or NaN
 *   argument, an angle above pi: HRY_E_ARG. */
typedef struct hry_normal_error {
    double   max_chord;    /* largest chord over the compared faces; 0 when there is none */
    double   sum_sq_chord; /* sum of c2 over the compared faces */
    uint64_t compared, skipped, nonfinite, degenerate, collapsed;
    uint32_t argmax;       /* lowest face attaining max_chord; HRY_NO_ELEMENT when compared == 0 */
    int32_t  list;         /* the position list; -1 (everything else 0): no normals, hry_last_error says why */
} hry_normal_error;        /* 64 bytes */
int  hry_chord_angle(double chord, double *radians);
int  hry_angle_chord(double radians, double *chord);
/* hry_distortion_build with HRY_DISTORTION_NORMALS: face f of a is taken twice, N_x from a's positions, N_y from b's at the mapped
 *   rows -- the "vertex" / "list<l>" map the build checks into its status word anyway.  Only a's connectivity is read, so b's
 *   numbering of faces never matters.  With HRY_DISTORTION_ROWS too the handle carries "normal_error", f32 [faces]: (float) chord of a
 *   compared face, 0 elsewhere.  a's connectivity is read in place when a is ctx's resident mesh, otherwise it goes up and counts in
 *   uploaded_bytes; an all-triangle mesh reads no face offsets.
 *   Refusals: a mesh without a position list of three POS components, without faces, or with a vertex region that does not bind
 *   the list gives list -1 with the reason -- it never fails a build that would have succeeded without the flag.
 * hry_distortion_normals: the record; list -1 also when the flag was not set. */
#define HRY_DISTORTION_NORMALS 4u   /* also the normal deviation per face (hry_distortion_normals) */
int  hry_distortion_normals(const hry_distortion *d, hry_normal_error *out);
/* hry_quant_sweep_build_ex with HRY_SWEEP_NORMALS: where the positions are swept (hry_quant_sweep_position has rows 1 .. pos_qmax),
 *   one record per width: field for field what hry_distortion_normals gives for q = hry_mesh_clone(m), hry_requant(ctx, q, {the three
 *   position components at bits}, 3, 0), hry_distortion_build(ctx, m, q, NULL, HRY_DISTORTION_NORMALS) -- up to the association of
 *   sum_sq_chord.  Residency follows the sweep's: the resident mesh's records and connectivity are read in place, otherwise they go
 *   up into the build's working buffer.  Flags 0 is hry_quant_sweep_build, launch for launch; unknown bits: HRY_E_ARG.
 * hry_quant_sweep_normals: the record at `bits` (outside 1 .. pos_qmax: HRY_E_ARG).  A sweep built without the flag:
 *   HRY_E_UNSUPPORTED, "the normals were not swept".  Built with it where the normals could not be swept (positions not all swept, no
 *   faces, a vertex region that does not bind the position list): HRY_OK, list -1, hry_last_error says why.
 * HRY_TOL_NORMAL_CHORD in hry_quant_choose: comp must be -1 and list the position list, like HRY_TOL_POS_DIST; one width for the three
 *   position components, met at `bits` when max_chord <= value AND collapsed == 0 at that width (a face that lost its normal has no
 *   angle to be within).  A sweep built without the flag, or whose normals were not swept: HRY_E_UNSUPPORTED. */
#define HRY_SWEEP_NORMALS 1u       /* (hry_quant_sweep_build_ex and hry_quant_sweep_normals: declared with the sweep, below) */

/* ---- a quantisation from a tolerance: the error at every bit width in one pass, on the device --------------------------
 * hry_quant_sweep_build reads every unquantised component of m once and, in registers, takes each value through hry_requant's
 * quantiser and the -c dequantiser at every width it can have: a table of hry_comp_error records per (list, component, bits).
 * hry_quant_choose turns tolerances into the hry_quant requests that meet them, ready for hry_requant.
 *   Swept: the lists hry_distortion_build compares; of them every component with 0 quantisation bits that hry_requant accepts, at
 *     every width 1 .. qmax = min(30, 8 * sizeof(type)).  Not swept (hry_quant_sweep_bits 0, hry_last_error says why): a component
 *     that is already quantised, one that hry_requant refuses (a constant integer component, a signed one over its type's whole
 *     range), and the components of a list that is not compared.
 *   Equivalence to the loop it replaces: with q = hry_mesh_clone(m), hry_requant(ctx, q, {l, c, bits}, 1, 0) and
 *     hry_distortion_build(ctx, m, q, NULL, 0), the record of (l, c, bits) equals hry_distortion_component(l, c) of that build
 *     field for field (skipped is 0), up to the association of sum_sq.  The arithmetic is hry_requant's own, not a closed form:
 *     floats are evaluated in float, integers through the reference's wrapping rescale, the extent is shared over an
 *     interpretation group.  The table therefore need not be monotone in bits.
 *   Positions: for the position list of hry_distortion_build, when its three position components are all swept, one hry_pos_error
 *     per width 1 .. the least of their qmax: what that build's hry_distortion_position gives with all three quantised to `bits`.
 *   max_abs, argmax, a_min, a_max and the counters are exact.  sum_sq has the same bits from run to run and whether m was resident
 *     or uploaded: a reduction tree fixed by the row count alone, no floating-point atomics.
 *   Bounds: where a list of m has none they are computed first, exactly as hry_requant does (m becomes ctx's resident mesh, and
 *     what ctx held of a decode is gone).  With the bounds known nothing is disturbed: when m is ctx's resident mesh
 *     (hry_mesh_resident) its records are read in place, otherwise they go up into the build's own working buffer
 *     (uploaded_bytes); the resident mesh and the buffers of a decode stay what they were.
 *   Refusals: a partial mesh, a list without its records: HRY_E_ARG; more than 16 lists, more than 32 components in a compared
 *     list: HRY_E_UNSUPPORTED.  *out stays NULL and ctx stays usable.
 *   The handle holds the host table only: no device memory.  It may outlive the context.
 *   hry_quant_sweep_bits       qmax of component c of list l; 0: not swept (hry_last_error: why); a bad l or c: HRY_E_ARG
 *   hry_quant_sweep_component  the record at `bits`; bits outside 1 .. qmax, a bad l or c: HRY_E_ARG; not swept: HRY_E_UNSUPPORTED
 *   hry_quant_sweep_position   the positions' record at `bits` (outside 1 .. the least qmax of the three: HRY_E_ARG); list -1,
 *                              everything else 0: the mesh has no positions, or they are not all swept
 *   hry_quant_sweep_stat       device_ms: the two kernels, by events; uploaded_bytes: the records that went up
 * hry_quant_choose, host only, on the table.  Per component that a tolerance names the request is the SMALLEST bits whose record
 * meets every tolerance on that component AT THAT WIDTH -- the table need not be monotone, so a wider width is not promised to:
 *     HRY_TOL_MAX_ABS   max_abs <= value
 *     HRY_TOL_MAX_REL   max_abs <= value * extent; extent: the component's shared extent (the scale hry_requant divides by), as a double
 *     HRY_TOL_RMS       sqrt(sum_sq / compared) <= value; not met when compared == 0
 *     HRY_TOL_POS_DIST  comp must be -1 and list the position list: one width for the three position components, max_dist <= value
 *   comp -1: every swept component of the list.  Requests come in the order the tolerances first name their components; *n_out is
 *   their number, also when cap is too small (HRY_E_ARG, nothing written).  No width meets the tolerances: the request is bits 0
 *   (the component stays lossless) -- but for HRY_DOUBLE, which cannot be coded lossless: HRY_E_UNSUPPORTED, naming list and component.
 *   A negative or NaN value, an unknown metric, a bad list or component, POS_DIST on another list or with a comp: HRY_E_ARG.  A
 *   component named that was not swept (positions that were not): HRY_E_UNSUPPORTED with the stored reason.
 * hry_quant_pick, host only, needs no device and no handle: the smallest bits in 1 .. n_bits whose record by_bits[bits - 1] meets
 *   (metric, value), 0: none does; HRY_TOL_POS_DIST, a negative or NaN value, n_bits < 0: HRY_E_ARG. */
typedef struct hry_sweep hry_sweep;
int  hry_quant_sweep_build(hry_ctx *ctx, hry_mesh *m, hry_sweep **out);
int  hry_quant_sweep_build_ex(hry_ctx *ctx, hry_mesh *m, uint32_t flags /* HRY_SWEEP_* */, hry_sweep **out);
int  hry_quant_sweep_normals(const hry_sweep *s, int bits, hry_normal_error *out);
int  hry_quant_sweep_bits(const hry_sweep *s, int l, int c);
int  hry_quant_sweep_component(const hry_sweep *s, int l, int c, int bits, hry_comp_error *out);
int  hry_quant_sweep_position(const hry_sweep *s, int bits, hry_pos_error *out);
int  hry_quant_sweep_stat(const hry_sweep *s, double *device_ms, uint64_t *uploaded_bytes);
void hry_quant_sweep_free(hry_sweep *s);
enum { HRY_TOL_MAX_ABS = 0, HRY_TOL_MAX_REL = 1, HRY_TOL_RMS = 2, HRY_TOL_POS_DIST = 3 };
enum { HRY_TOL_NORMAL_CHORD = 4 };   /* hry_quant_choose on a sweep with HRY_SWEEP_NORMALS (section 7h, above) */
typedef struct hry_tolerance {
    int32_t list;
    int32_t comp;          /* -1: every swept component of the list */
    int32_t metric;        /* HRY_TOL_* */
    int32_t reserved;
    double  value;
} hry_tolerance;
int  hry_quant_choose(const hry_sweep *s, const hry_tolerance *t, size_t nt, hry_quant *out, size_t cap, size_t *n_out);
int  hry_quant_pick(const hry_comp_error *by_bits /* [n_bits], index bits - 1 */, int n_bits, int metric, double extent, double value);

/* ---- the coded size at every quantisation width ------------------------------------------------
 * The other column of a lossy encode: what every width of a vertex attribute costs in bytes, from one pass over the coding order,
 * where the loop it replaces clones, requantises and encodes the mesh once per width.
 * hry_rate_sweep_build: PLY layout only -- general bindings are HRY_E_UNSUPPORTED with that reason, a partial mesh HRY_E_ARG.  Only
 *   list 1, the vertex list, is swept (face records are coded against a zero prediction): for a component of another list
 *   hry_rate_sweep_bits is 0 and the reason is stored.  Widths 1 .. qmax are swept for exactly the components of list 1 that
 *   hry_quant_sweep_bits reports as swept, with the same qmax (one test serves both).  Row bits == 0 is the component as it stands: it
 *   is there for every component of list 1 that hry_encode codes as stored, quantised ones included; a lossless HRY_DOUBLE has none
 *   (HRY_E_UNSUPPORTED with the encoder's own text).
 *   The table is the encoder's, not a model of it: hist(l, c, bits, p)[s] is the number of coded vertices whose byte p of the
 *   residual code of component c equals s, the code being the one hry_encode writes into its "vplanes" stage for a clone q =
 *   hry_mesh_clone(m) after hry_requant(ctx, q, {l, c, bits}, 1, 0) -- for row 0, for m itself -- in either profile (the planes are
 *   the same).  Planes of a component are counted from its first plane; there are sizeof(storage type) of them: u8 up to 8 bits, u16
 *   up to 16, u32 above.  The components of a vertex are predicted independently, so the table of c also holds when other components
 *   are quantised at the same time.  Counts are exact, and every histogram sums to hry_rate_sweep_coded: the length of the walk's
 *   "order_v", not the vertex count -- vertices no face names are not coded.  A mesh without faces: coded == 0, all histograms zero,
 *   all bytes 0, no error.
 *   The walk is the encoder's own (hry_walk_run_plain's loop): it leaves m's twins exactly as hry_encode leaves them; m becomes ctx's
 *   resident mesh as by hry_mesh_upload if it was not; bounds are computed first where missing, as hry_requant does.  Nothing else of
 *   m changes: hry_encode(m) afterwards gives the bytes it gave before.  The handle holds the host table only and may outlive the
 *   context; on any refusal *out stays NULL and ctx stays usable.
 * hry_rate_sweep_planes: the byte planes of (l, c) at that width: 1, 2 or 4 (row 0: of the storage type as it stands, 8 for a lossless
 *   64-bit integer); a bad list,
 *   component or width: HRY_E_ARG; a component or row that is not there: HRY_E_UNSUPPORTED with the stored reason.  _hist and _bytes
 *   refuse the same way, _hist a plane outside [0, planes) with HRY_E_ARG.
 * hry_rate_hist_bytes, host only: with n = sum(hist), (sum over s in ascending order with hist[s] > 0 of hist[s] * log2(n / hist[s]))
 *   / 8, summed in double; 0 when n == 0 or one symbol holds everything (such a plane carries no information and the container does
 *   not store it).
 * hry_rate_sweep_bytes: the sum of hry_rate_hist_bytes over the component's planes in plane order.  An ESTIMATE of the attribute
 *   payload and nothing else: not the models' adaptation, the chunks' priors, the directory or the connectivity.
 * hry_rate_pick, host only: the LARGEST bits in 1 .. n_bits with bytes_by_bits[bits - 1] <= budget, 0: none -- the mirror of
 *   hry_quant_pick.  The table need not be monotone: nothing is promised about narrower widths.  A negative or NaN budget, n_bits < 0:
 *   HRY_E_ARG.
 * hry_rate_choose: hry_rate_pick over the per-width sums of hry_rate_sweep_bytes of the named components (c -1: every swept component
 *   of l, ONE common width), at widths up to the least of their qmax; *bits 0: none fits; *bytes (may be NULL): the sum at *bits.  A
 *   named component that is not swept, or a list without a swept one: HRY_E_UNSUPPORTED with the stored reason.
 * hry_rate_sweep_stat: device_ms (the sweep kernel, by events), walk_ms (the host's walk), uploaded_bytes (a mesh that was not
 *   resident; where the bounds had to be computed first the mesh went up for them, and this is 0). */
typedef struct hry_rate_sweep hry_rate_sweep;
int      hry_rate_sweep_build(hry_ctx *ctx, hry_mesh *m, hry_rate_sweep **out);
uint32_t hry_rate_sweep_coded(const hry_rate_sweep *s);                       /* coded vertices = symbols per plane */
int      hry_rate_sweep_bits(const hry_rate_sweep *s, int l, int c);          /* qmax; 0: not swept (hry_last_error: why) */
int      hry_rate_sweep_planes(const hry_rate_sweep *s, int l, int c, int bits);
int      hry_rate_sweep_hist(const hry_rate_sweep *s, int l, int c, int bits, int plane, uint32_t out[256]);
int      hry_rate_sweep_bytes(const hry_rate_sweep *s, int l, int c, int bits, double *out);
int      hry_rate_sweep_stat(const hry_rate_sweep *s, double *device_ms, double *walk_ms, uint64_t *uploaded_bytes);
void     hry_rate_sweep_free(hry_rate_sweep *s);
int      hry_rate_hist_bytes(const uint32_t hist[256], double *out);
int      hry_rate_pick(const double *bytes_by_bits /* [n_bits], index bits - 1 */, int n_bits, double budget);
int      hry_rate_choose(const hry_rate_sweep *s, int l, int c, double budget, int *bits, double *bytes);

/* ---- one mesh over several GPUs ---------------------------------------------------- */
/* The reference has no multi-device path; what a split must honour is its numbering: vertices, faces and half-edges of the
 * decoded mesh are numbered in coding order across ALL connected components (cbm/encoder.h:61-68,215; cbm/decoder.h:48,75,
 * 145,162), components that share a vertex name it by that number (cbm/encoder.h:79-113,187), and the order of the
 * components is the start-face sequence over the whole mesh (formats/hry/writer.cc:28-46).
 *   hry_shard_plan     host analysis of the connectivity (no walk): components, their coding order, groups of components tied
 *                      by shared vertices, exclusive scans of the vertices / faces / half-edges each introduces, and the
 *                      distribution of the groups over n_shards (balanced by triangle count).  Deterministic: every rank
 *                      that holds the mesh computes the same plan.
 *   hry_shard_extract  the sub-mesh of one shard in its own compact numbering; it carries the seed face of each of its
 *                      components and the place of its runs of components in the whole numbering.  hry_encode (CHUNKED) of
 *                      a shard writes a one-segment sharded container (.hry v0.3) whose header describes the WHOLE mesh:
 *                      give the shard the bounds of the whole mesh first (hry_list_set_bounds) -- they are in that header
 *                      and scale the quantisation (structs/quant.h:30-96).
 *   hry_merge          concatenates the segments of several such containers into ONE .hry v0.3 (no re-coding).
 *   hry_decode         reads it on one GPU (all segments) or, with opts->shard_index / shard_count, a share of the segments
 *                      per process; hry_mesh_runs lists the runs of the whole numbering that the returned mesh holds. */
typedef struct hry_plan hry_plan;
int hry_shard_plan(const hry_mesh *m, int n_shards, hry_plan **out);
void hry_plan_free(hry_plan *p);
uint32_t hry_plan_ncomponents(const hry_plan *p);
uint32_t hry_plan_ngroups(const hry_plan *p);
uint64_t hry_plan_triangles(const hry_plan *p, int shard);
int hry_shard_extract(const hry_mesh *m, const hry_plan *p, int shard, hry_mesh **out);
int hry_merge(const uint8_t *const *parts, const size_t *sizes, size_t n, uint8_t **out, size_t *out_len);
/* runs as 6 x u32 each: first_vertex, first_face, first_halfedge, n_vertices, n_faces, n_halfedges (numbering of the whole
 * mesh).  For a shard: where its components go; for a mesh decoded from a sharded container: what was decoded. */
size_t hry_mesh_runs(const hry_mesh *m, const uint32_t **runs);
/* for a shard: index in the whole mesh of every vertex (which = 1) / face (which = 0) of the shard; which = 2: the start face of
 * each of its components (shard numbering) in coding order; which = 16 + l (general bindings): index in the whole mesh of every
 * record of list l */
size_t hry_shard_elements(const hry_mesh *m, int which, const uint32_t **idx);
/* bounds of a list as records in the original component types (what hry_list_min / hry_list_max return) */
int hry_list_set_bounds(hry_mesh *m, int l, const uint8_t *min_rec, const uint8_t *max_rec);
/* after hry_bounds: 1 + index of the first element that holds the minimum / maximum of component c, 0 = the initial value of
 * the reference's scan (structs/quant.h:33) -- what a combination of per-shard bounds needs to break ties (+-0.0) like one scan */
uint32_t hry_list_min_at(const hry_mesh *m, int l, int c);
uint32_t hry_list_max_at(const hry_mesh *m, int l, int c);
int hry_mesh_partial(const hry_mesh *m);   /* 1: decoded with HRY_FLAG_PARTIAL / as a share; only its runs are real */

/* ---- the same from ONE process over several devices ---------------------------------------------------------------
 * The reference's single entry (main.cc:93-123 -> quant::requant -> hry::writer::write, formats/hry/writer.cc:200-214) with
 * N device contexts behind it: what scales is "host thread + context" (the sequential cut-border walk of a shard on a host
 * core, the kernels of that shard on the context's device), so every context gets a worker thread of its own, confined to the
 * memory node of its device.  Contexts may sit on different devices (one per GPU of a node) or share one.
 *   hry_encode_sharded  plans once, extracts the shards on the workers, combines the shards' k_bounds results into the bounds of
 *                       the whole mesh with the tie rule of ONE scan (structs/quant.h:30-44), quantises (quant / n_quant / clear
 *                       as hry_requant; the shards are quantised, *m keeps its values and receives the bounds) and codes every
 *                       shard (CHUNKED) on its worker, and concatenates the segments in host memory: ONE .hry v0.3, byte-identical
 *                       to hry_shard_plan / hry_shard_extract / hry_encode / hry_merge run shard by shard.  opts->shard_count =
 *                       number of shards (0: one per context); shard s is coded by context s % n_ctx.
 *   hry_decode_sharded  decodes the segments of a sharded container on the contexts (segment i on context i % n_ctx) into ONE
 *                       mesh in the numbering of the whole; opts->shard_index / shard_count select a share as in hry_decode.
 * hry_ctx_timing of each context holds the sums over the shards / segments it processed. */
typedef struct hry_shard_timing {
    double twins_ms;     /* encode: half-edge twin matching of a freshly read mesh (first context's device), part of plan_ms */
    double plan_ms;      /* encode: twins + components + coding order + scans + distribution; decode: directory checks */
    double extract_ms;   /* encode: hry_shard_extract (decode: placement into the whole numbering), max over the workers */
    double bounds_ms;    /* upload + k_bounds per shard, max over the workers */
    double combine_ms;   /* bounds of the whole mesh from the shards' */
    double quant_ms;     /* quantisation: of the whole lists on the first context (device plan), of the extracted shards (max over the workers); coded in place on other devices it is part of extract_ms */
    double encode_ms;    /* hry_encode (decode: the segments' decode), max over the workers */
    double merge_ms;     /* concatenation of the segments (decode: filler for what no decoded run covers) */
    double phase_a_ms;   /* wall clock: extraction + bounds on all workers */
    double phase_b_ms;   /* wall clock: quantisation + encode (decode: decode + placement) on all workers */
    double host_walk_ms; /* the longest worker's cut-border walks / replays */
    double total_ms;
    uint32_t n_shards, n_contexts, n_segments, n_components, n_groups;
} hry_shard_timing;
int hry_encode_sharded(hry_ctx *const *ctx, int n_ctx, hry_mesh *m, const hry_quant *quant, size_t n_quant, int clear,
                       const hry_opts *opts, uint8_t **out, size_t *out_len, hry_shard_timing *timing /* may be NULL */);
int hry_decode_sharded(hry_ctx *const *ctx, int n_ctx, const uint8_t *hry, size_t n, const hry_opts *opts, hry_mesh **out,
                       hry_shard_timing *timing /* may be NULL */);
/* host-only: the directory of a sharded container checked against its header (segment extents, run tables, runs inside the mesh,
 * no overlap, order of faces and half-edges consistent); *complete = every face and half-edge lies in some run */
int hry_container_check(const uint8_t *hry, size_t n, int *complete);

/* ---- stage-level access for parity tests (valid after hry_encode/hry_decode with keep_stages) ----- */
/* names: "order_v","order_f","twin","vplanes","fplanes","rec","sym_l","r","S","payload","dec_syms","dec_nsym","enc_plan","dec_plan",
 * ... */
int hry_stage_get(hry_ctx *ctx, const char *name, void **host_copy, size_t *bytes);

/* host-only: the sequential cut-border walk of the encoder (cbm::encode, cbm/encoder.h:54-217) with a recording
 * writer.  Mutates the mesh's twins like hry_encode.  Arrays by name: "order_v", "order_f", "op_sym"(u8), "op_class"(u8),
 * "op_l", "op_h", "op_t", "op_pos", "grp<k>_val", "grp<k>_pos" with k = 0 iop, 1 elem, 2 part, 3 vertid, 4 numtri
 * (u32 unless noted), "info" = { n_conn, numtri_coded }.  hry_walk_get returns the element count. */
typedef struct hry_walk hry_walk;
int hry_walk_run(hry_mesh *m, hry_walk **out);
/* same walk without evaluating the operation model (what the chunked profile uses; then "op_l/op_h/op_t/op_pos" are empty and
 * components after the first may be walked on several host threads: HRY_HOST_THREADS, default min(16, cores)) */
int hry_walk_run_plain(hry_mesh *m, hry_walk **out);
/* host-only: the components of shard `shard` of a plan (hry_shard_plan), walked where they lie in the whole mesh -- what a worker
 * of hry_encode_sharded does instead of walking an extracted sub-mesh: same symbols as hry_walk_run_plain of hry_shard_extract's
 * mesh, "order_v" / "order_f" as half-edges of the WHOLE mesh.  Mutates the mesh's twins like hry_encode. */
int hry_walk_run_shard(hry_mesh *m, const hry_plan *plan, int shard, hry_walk **out);
/* development / tests: the component analysis of the mesh (connected components, coding order, sizes, new vertices, ties -- what
 * hry_encode of a large mesh computes on the device before its walk, analysis.cpp) by the device AND by the host, compared table by
 * table; 0 = equal (or fewer than two components), HRY_E_INTERNAL with the first difference otherwise.  Uploads the mesh. */
int hry_analysis_check(hry_ctx *ctx, hry_mesh *m);
/* development / tests: that analysis as arrays by name, from either side -- on_device 0: the host's (ctx may be NULL, no GPU is touched),
 * 1: the device's (uploads the mesh unless it is resident; a mesh of one component gets its tables too, which an encode never asks
 * for).  Read with hry_walk_get (u32), free with hry_walk_free: "ncomp" (one word); per coding rank "by_rank", "seed", "n_faces",
 * "n_halfedges", "fresh", "group", "face_lo", "face_hi", "vtx_lo", "vtx_hi"; "comp" = the component number of every face (on the device
 * the label words, copied down for this call only); "spans" = the start-face sequence of nf faces as (lowest face, highest face,
 * position of the span's first face, 1 = ascending) sorted by the lowest face; on_device only: "twin_over" (one word) = how many
 * vertices the device's twin matching left to the host when this mesh's twins were matched (0: none, up to 4096: those vertices
 * were matched on the host, above: the host matched everything; 0xffffffff: the twins were never matched on a device). */
int hry_analysis_tables(hry_ctx *ctx, hry_mesh *m, int on_device, hry_walk **out);
size_t hry_walk_get(const hry_walk *w, const char *name, const void **ptr);
void hry_walk_free(hry_walk *w);

/* host-only: the serial half of reading a reference stream (.hry v0.1): entropy decoding of the single adaptive
 * stream interleaved with the cut-border replay (hry::reader::read, formats/hry/reader.cc:179-193; cbm::decode,
 * cbm/decoder.h:27-211; arith/coder.h:115-172).  *mesh gets the connectivity (attribute records still zero); the
 * result holds "order_v" (u32, decode order as half-edges), "vplanes"/"fplanes" (u8, residual byte planes, plane-major)
 * for the device reconstruction.  Free with hry_walk_free / hry_mesh_free. */
int hry_stream_read_host(const void *hry, size_t bytes, hry_mesh **mesh, hry_walk **out);

/* host-only: the decoder-side cut-border replay (cbm::decode, cbm/decoder.h:27-211) of the connectivity symbols a plain
 * walk recorded, as the chunked container carries them (21 byte planes).  use_restart_points 1: cut the replay at the
 * restart points the container directory would hold and replay the spans on several host threads (HRY_HOST_THREADS,
 * HRY_PARALLEL_MIN_FACES); 3: also at the border snapshots INSIDE the components (what hry_walk_run_plain noted every
 * HRY_SNAPSHOT_FACES faces of a component; through the directory's form and back): spans with placeholders for the border's
 * half-edges, joined afterwards.  *mesh gets nv/nf and the rebuilt connectivity; the result holds "order_v", "seg_start",
 * "seg_level" (u32) and "info" = { number of restart points, number of border snapshots }; hry_walk_get(walk, "snap_section")
 * is the directory section of a walk's snapshots. */
int hry_walk_replay(const hry_mesh *src, const hry_walk *walk, int use_restart_points, hry_mesh **mesh, hry_walk **out);

/* raw range-coder back end on explicit (l,h,t) triples (arith/coder.h:69-91 + flush :58-67), compat form */
int hry_range_encode_lht(hry_ctx *ctx, const uint64_t *lht, size_t n, uint8_t **out, size_t *out_len);

#ifdef __cplusplus
}
#endif
#endif
