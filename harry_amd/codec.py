"""Host-side mirror of the reference's interface for the .hry path, on top of the C ABI (include/harry_amd.h).

Reference seams mirrored here (names and argument meaning follow the reference):
    unified::reader::read(fn, mesh)      formats/unified_reader.h:78-86   -> read_mesh(path)
    quant::requant(attrs, quants, clear) structs/quant.h:222-242          -> Codec.requant(mesh, quants, clear)
    hry::writer::write(os, mesh)         formats/hry/writer.h:19          -> Codec.write_hry(mesh)
    hry::reader::read(is, mesh)          formats/hry/reader.h:19          -> Codec.read_hry(data)
    ply::writer::write(os, mesh, ascii)  formats/ply/writer.cc:136-192    -> Mesh.to_ply(ascii)

All computation happens in libharry_amd.so (host C++ for the walk / PLY I/O, HIP kernels for the rest).
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _native as nat
from ._native import FLAG_DEVICE_RECURRENCE, FLAG_HOST_RECURRENCE, FLAG_KEEP_MESH, FLAG_ORDER, FLAG_PARTIAL, NO_ELEMENT, HryError, PROFILE_CHUNKED, PROFILE_COMPAT  # noqa: F401

TYPE_NP = {0: "<f4", 1: "<f8", 2: "<u8", 3: "<i8", 4: "<u4", 5: "<i4", 6: "<u2", 7: "<i2", 8: "u1", 9: "i1"}
TYPE_SIZE = {0: 4, 1: 8, 2: 8, 3: 8, 4: 4, 5: 4, 6: 2, 7: 2, 8: 1, 9: 1}
NP_TYPE = {"f4": 0, "f8": 1, "u8": 2, "i8": 3, "u4": 4, "i4": 5, "u2": 6, "i2": 7, "u1": 8, "i1": 9}


def storage_type(t: int, q: int) -> int:
    """structs/mixing.h:101-108"""
    if q == 0:
        return t
    return 8 if q <= 8 else 6 if q <= 16 else 4 if q <= 32 else 2


class Mesh:
    """In-memory mesh (reference: mesh::Mesh, structs/mesh.h:19-40) as flat arrays owned by the native library."""

    def __init__(self, handle):
        self.h = handle

    def __del__(self):
        if getattr(self, "h", None):
            nat.load().hry_mesh_free(self.h)
            self.h = None

    # ---- construction
    @classmethod
    def from_ply(cls, data: bytes) -> "Mesh":
        h = C.c_void_p()
        nat.check(nat.load().hry_mesh_from_ply(data, len(data), C.byref(h)))
        return cls(h)

    @classmethod
    def from_obj(cls, data: bytes, directory: str = "") -> "Mesh":
        """OBJ text -> mesh with general bindings (regions, shared records, corner lists); `directory`: where "mtllib" files are"""
        h = C.c_void_p()
        nat.check(nat.load().hry_mesh_from_obj(data, len(data), directory.encode(), C.byref(h)))
        return cls(h)

    @classmethod
    def from_arrays(cls, verts: np.ndarray, degrees: np.ndarray, indices: np.ndarray, face_props: np.ndarray | None = None) -> "Mesh":
        """verts / face_props: numpy structured arrays (packed), one field per component."""
        L = nat.load()

        def pack(a):
            if a is None or a.dtype.names is None or len(a.dtype.names) == 0:
                return None, 0, None, None, []
            names = list(a.dtype.names)
            packed = np.empty(len(a), dtype=np.dtype([(n, a.dtype[n].newbyteorder("<")) for n in names]))
            for n in names:
                packed[n] = a[n]
            types = np.array([NP_TYPE[a.dtype[n].str[1:]] for n in names], np.uint8)
            cn = (C.c_char_p * len(names))(*[n.encode() for n in names])
            return packed, len(names), types, cn, names

        vp, vn, vt, vnames, _ = pack(verts)
        fp, fn, ft, fnames, _ = pack(face_props)
        degrees = np.ascontiguousarray(degrees, np.uint8)
        indices = np.ascontiguousarray(indices, np.uint32)
        h = C.c_void_p()
        nat.check(L.hry_mesh_from_arrays(
            len(verts), vp.ctypes.data if vp is not None else None, vn, vt.ctypes.data if vt is not None else None, vnames,
            len(degrees), degrees.ctypes.data, indices.ctypes.data,
            fp.ctypes.data if fp is not None else None, fn, ft.ctypes.data if ft is not None else None, fnames, C.byref(h)))
        return cls(h)

    def clone(self) -> "Mesh":
        h = nat.load().hry_mesh_clone(self.h)
        if not h:
            raise MemoryError("hry_mesh_clone")
        return Mesh(C.c_void_p(h))

    def flip_faces(self, face_flip) -> "Mesh":
        """a clone in which every face f with face_flip[f] != 0, (v0, v1, ..., vk-1), is (v0, vk-1, ..., v1); per-corner records follow
        their corners (hry_mesh_flip_faces).  face_flip: nf values, for instance "face_flip" of Codec.orient / orient_numpy"""
        if hasattr(face_flip, "detach"):   # a torch tensor
            face_flip = face_flip.detach().cpu().numpy()
        flags = np.ascontiguousarray(np.asarray(face_flip).reshape(-1) != 0, dtype=np.uint32)
        if len(flags) != self.nf:
            raise HryError(nat.E_ARG, "face_flip needs one value per face")
        h = C.c_void_p()
        nat.check(nat.load().hry_mesh_flip_faces(self.h, flags.ctypes.data, C.byref(h)))
        return Mesh(h)

    # ---- accessors
    nv = property(lambda s: nat.load().hry_mesh_nv(s.h))
    nf = property(lambda s: nat.load().hry_mesh_nf(s.h))
    ne = property(lambda s: nat.load().hry_mesh_ne(s.h))
    ntri = property(lambda s: nat.load().hry_mesh_ntri(s.h))

    def face_offsets(self):
        return nat.arr(nat.load().hry_mesh_face_offsets(self.h), self.nf + 1, np.uint32)

    def org(self):
        return nat.arr(nat.load().hry_mesh_org(self.h), self.ne, np.uint32)

    def twin(self):
        return nat.arr(nat.load().hry_mesh_twin(self.h), self.ne, np.uint32)

    def list_fmt(self, l):
        L = nat.load()
        return [(L.hry_list_type(self.h, l, c), L.hry_list_quant(self.h, l, c), L.hry_list_offset(self.h, l, c))
                for c in range(L.hry_list_ncomp(self.h, l))]

    def list_stride(self, l):
        return nat.load().hry_list_stride(self.h, l)

    def list_count(self, l):
        return nat.load().hry_list_count(self.h, l)

    def list_data(self, l) -> np.ndarray:
        n, s = self.list_count(l), self.list_stride(l)
        if n * s == 0:
            return np.zeros((n, s), np.uint8)
        return nat.arr(nat.load().hry_list_data(self.h, l), n * s, np.uint8).reshape(n, s)

    def list_min(self, l):
        p = nat.load().hry_list_min(self.h, l)
        return nat.arr(p, self.list_stride(l), np.uint8) if p else None

    def list_max(self, l):
        p = nat.load().hry_list_max(self.h, l)
        return nat.arr(p, self.list_stride(l), np.uint8) if p else None

    def component(self, l, c) -> np.ndarray:
        t, q, off = self.list_fmt(l)[c]
        st = storage_type(t, q)
        return self.list_data(l)[:, off:off + TYPE_SIZE[st]].copy().view(TYPE_NP[st]).reshape(-1)

    def set_bounds(self, l: int, mn: bytes, mx: bytes):
        """bounds of list l as records in the original component types (the whole mesh's, for a shard)"""
        nat.check(nat.load().hry_list_set_bounds(self.h, l, bytes(mn), bytes(mx)))

    def bounds_at(self, l: int):
        """after Codec.bounds: per component (1 + index of the first element holding the minimum, same for the maximum); 0 = the
        initial value of the reference's scan"""
        L = nat.load()
        n = L.hry_list_ncomp(self.h, l)
        return [(L.hry_list_min_at(self.h, l, c), L.hry_list_max_at(self.h, l, c)) for c in range(n)]

    partial = property(lambda s: bool(nat.load().hry_mesh_partial(s.h)))

    def runs(self) -> np.ndarray:
        """(n, 6) u32: first_vertex, first_face, first_halfedge, n_vertices, n_faces, n_halfedges in the numbering of the whole mesh.
        A shard: where its components go.  A mesh decoded from a sharded container: what was decoded."""
        p = C.c_void_p()
        n = nat.load().hry_mesh_runs(self.h, C.byref(p))
        if n == 0:
            return np.zeros((0, 6), np.uint32)
        return np.frombuffer(C.string_at(p, n * 24), dtype=np.uint32).reshape(n, 6).copy()

    def shard_elements(self, which: int) -> np.ndarray:
        """a shard: index in the whole mesh of every vertex (which = 1) / face (which = 0)"""
        p = C.c_void_p()
        n = nat.load().hry_shard_elements(self.h, which, C.byref(p))
        return np.frombuffer(C.string_at(p, n * 4), dtype=np.uint32).copy() if n else np.zeros(0, np.uint32)

    def to_ply(self, ascii: bool = False, packed: bool = False) -> bytes:
        """packed: quantised components in the width of the storage type the header declares (see HRY_PLY_PACKED)"""
        p, n = C.c_void_p(), C.c_size_t()
        nat.check(nat.load().hry_mesh_to_ply(self.h, int(ascii) | (2 if packed else 0), C.byref(p), C.byref(n)))
        return nat.take_bytes(p, n.value)

    def to_obj(self) -> bytes:
        p, n = C.c_void_p(), C.c_size_t()
        nat.check(nat.load().hry_mesh_to_obj(self.h, 0, C.byref(p), C.byref(n)))
        return nat.take_bytes(p, n.value)

    # ---- general bindings (structs/attr.h:101-189)
    general = property(lambda s: bool(nat.load().hry_mesh_general(s.h)))
    nlists = property(lambda s: nat.load().hry_mesh_nlists(s.h))

    def list_target(self, l) -> int:
        return nat.load().hry_list_target(self.h, l)

    def nregions(self, which: int) -> int:
        return nat.load().hry_mesh_nregions(self.h, which)

    def region_lists(self, kind: int, r: int):
        out = np.zeros(256, np.uint16)
        n = nat.load().hry_mesh_region_lists(self.h, kind, r, out.ctypes.data, 256)
        return [int(x) for x in out[:n]]

    def regions_of(self, which: int) -> np.ndarray:
        p = C.c_void_p()
        n = nat.load().hry_mesh_regions_of(self.h, which, C.byref(p))
        return np.frombuffer(C.string_at(p, n * 2), dtype=np.uint16).copy() if n else np.zeros(0, np.uint16)

    def bindings(self, kind: int) -> np.ndarray:
        p, slots = C.c_void_p(), C.c_int()
        n = nat.load().hry_mesh_bindings(self.h, kind, C.byref(p), C.byref(slots))
        if not n or not slots.value:
            return np.zeros((n, slots.value), np.uint32)
        return np.frombuffer(C.string_at(p, n * slots.value * 4), dtype=np.uint32).copy().reshape(n, slots.value)

    def host_walk(self, plain: bool = False) -> dict:
        """Host-only cut-border walk with a recording writer (mutates twins like an encode).  plain: without the operation
        model (the chunked profile's walk; may use several host threads for multi-component meshes)."""
        L = nat.load()
        w = C.c_void_p()
        nat.check((L.hry_walk_run_plain if plain else L.hry_walk_run)(self.h, C.byref(w)))
        return _walk_arrays(w)


def _walk_arrays(w) -> dict:
    """every array of a recorded walk (hry_walk_get); frees the walk"""
    L = nat.load()
    try:
        out = {}
        names = [("order_v", np.uint32), ("order_f", np.uint32), ("op_sym", np.uint8), ("op_class", np.uint8), ("op_l", np.uint32),
                 ("op_h", np.uint32), ("op_t", np.uint32), ("op_pos", np.uint32), ("op_thr", np.uint32), ("op_cum", np.uint32), ("info", np.uint32),
                 ("marks", np.uint32), ("snap_section", np.uint8)]
        for g in range(5):
            names += [(f"grp{g}_val", np.uint32), (f"grp{g}_pos", np.uint32)]
        for name, dt in names:
            p = C.c_void_p()
            n = L.hry_walk_get(w, name.encode(), C.byref(p))
            out[name] = (np.frombuffer(C.string_at(p, n * np.dtype(dt).itemsize), dtype=dt).copy() if n else np.zeros(0, dt))
        return out
    finally:
        L.hry_walk_free(w)


ANALYSIS_TABLES = ("ncomp", "by_rank", "seed", "n_faces", "n_halfedges", "fresh", "group", "face_lo", "face_hi", "vtx_lo", "vtx_hi", "comp", "spans")


def _analysis_tables(ctx, mesh: Mesh, on_device: bool) -> dict:
    L = nat.load()
    w = C.c_void_p()
    nat.check(L.hry_analysis_tables(ctx, mesh.h, int(on_device), C.byref(w)))
    try:
        out = {}
        for name in ANALYSIS_TABLES + (("twin_over",) if on_device else ()):
            p = C.c_void_p()
            n = L.hry_walk_get(w, name.encode(), C.byref(p))
            out[name] = np.frombuffer(C.string_at(p, n * 4), dtype=np.uint32).copy() if n else np.zeros(0, np.uint32)
        out["spans"] = out["spans"].reshape(-1, 4)
        return out
    finally:
        L.hry_walk_free(w)


def analysis_tables_host(mesh: Mesh) -> dict:
    """Host-only: the component analysis of `mesh` as numpy arrays by name (hry_analysis_tables without a context; matches the twins
    on the host if they are pending)."""
    return _analysis_tables(None, mesh, False)


class ShardPlan:
    """Distribution of one mesh over n shards by groups of connected components (include/harry_amd.h, hry_shard_plan)."""

    def __init__(self, mesh: Mesh, n_shards: int):
        self.h = C.c_void_p()
        self.n_shards = n_shards
        nat.check(nat.load().hry_shard_plan(mesh.h, n_shards, C.byref(self.h)))

    def __del__(self):
        if getattr(self, "h", None):
            nat.load().hry_plan_free(self.h)
            self.h = None

    ncomponents = property(lambda s: nat.load().hry_plan_ncomponents(s.h))
    ngroups = property(lambda s: nat.load().hry_plan_ngroups(s.h))

    def triangles(self, shard: int) -> int:
        return nat.load().hry_plan_triangles(self.h, shard)

    def extract(self, mesh: Mesh, shard: int) -> Mesh:
        h = C.c_void_p()
        nat.check(nat.load().hry_shard_extract(mesh.h, self.h, shard, C.byref(h)))
        return Mesh(h)

    def walk_in_place(self, mesh: Mesh, shard: int) -> dict:
        """Host-only: the shard's components walked where they lie in `mesh` (hry_walk_run_shard; mutates its twins)."""
        w = C.c_void_p()
        nat.check(nat.load().hry_walk_run_shard(mesh.h, self.h, shard, C.byref(w)))
        return _walk_arrays(w)


def container_info(data: bytes) -> dict:
    """what a .hry file is, without decoding it (hry_container_info)"""
    info = (C.c_uint32 * 8)()
    nat.check(nat.load().hry_container_info(data, len(data), info))
    keys = ("minor", "header_bytes", "nv", "nf", "ne", "chunk_syms", "conn_chunk_syms", "segments")
    return dict(zip(keys, (int(x) for x in info)))


def merge(parts, as_buffer: bool = False):
    """several sharded containers (.hry v0.3) of the same mesh -> one (hry_merge).  The parts may be any buffers (bytes, numpy
    arrays, NativeBuffer): none is copied on the way in; as_buffer: the result stays in the library's buffer too."""
    where = [nat.buffer_address(p) for p in parts]
    arr = (C.c_void_p * len(parts))(*[w[0] for w in where])
    sizes = (C.c_size_t * len(parts))(*[w[1] for w in where])
    p, n = C.c_void_p(), C.c_size_t()
    nat.check(nat.load().hry_merge(arr, sizes, len(parts), C.byref(p), C.byref(n)))
    return nat.take(p, n.value, as_buffer)


def walk_and_replay(mesh: "Mesh", use_restart_points: bool):
    """Host-only: plain cut-border walk of `mesh` (mutates its twins), then the decoder-side replay of the recorded
    connectivity planes.  Returns (mesh with the rebuilt connectivity, order_v, seg_start, seg_level, n_restart_points)."""
    L = nat.load()
    w = C.c_void_p()
    nat.check(L.hry_walk_run_plain(mesh.h, C.byref(w)))
    try:
        mh, r = C.c_void_p(), C.c_void_p()
        nat.check(L.hry_walk_replay(mesh.h, w, int(use_restart_points), C.byref(mh), C.byref(r)))
        try:
            out = []
            for name in ("order_v", "seg_start", "seg_level", "info"):
                p = C.c_void_p()
                n = L.hry_walk_get(r, name.encode(), C.byref(p))
                out.append(np.frombuffer(C.string_at(p, n * 4), dtype=np.uint32).copy() if n else np.zeros(0, np.uint32))
            # use_restart_points: False / True (the restart points at component starts), or 2 / 3: + the border snapshots inside components
            return (Mesh(mh), out[0], out[1], out[2], int(out[3][0]) if int(use_restart_points) < 2 else (int(out[3][0]), int(out[3][1])))
        finally:
            L.hry_walk_free(r)
    finally:
        L.hry_walk_free(w)


def read_stream_host(data: bytes):
    """Host-only serial half of reading a reference (v0.1) stream: (mesh with connectivity, order_v, vplanes, fplanes)."""
    L = nat.load()
    mh, w = C.c_void_p(), C.c_void_p()
    nat.check(L.hry_stream_read_host(data, len(data), C.byref(mh), C.byref(w)))
    try:
        out = []
        for name, dt in (("order_v", np.uint32), ("vplanes", np.uint8), ("fplanes", np.uint8)):
            p = C.c_void_p()
            n = L.hry_walk_get(w, name.encode(), C.byref(p))
            out.append(np.frombuffer(C.string_at(p, n * np.dtype(dt).itemsize), dtype=dt).copy() if n else np.zeros(0, dt))
        return (Mesh(mh), *out)
    finally:
        L.hry_walk_free(w)


class _Chain:
    """The builds that lie behind one another on one codec and mesh (render, edges, ... : hry_<family>_build / _free).  build() keeps
    the handle it returns, so a later step names the earlier ones; leaving the `with` block frees what is still held, the last
    built first, each handle once, whatever happened.  lib: the native library, or anything with the same entry points"""

    def __init__(self, codec, mesh, lib=None):
        self.lib, self.codec, self.mesh = lib or nat.load(), codec, mesh
        self.held = []   # (family, handle) in the order of the builds

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()

    def build(self, family: str, *args, entry: str = ""):
        """hry_<family>_build (or `entry`) of the codec and the mesh with `args` between them and the new handle"""
        h = C.c_void_p()
        nat.check(getattr(self.lib, entry or f"hry_{family}_build")(self.codec.h, self.mesh.h, *args, C.byref(h)))
        self.held.append((family, h))
        return h

    def free(self, keep_last: bool = False):
        """free every handle held in reverse order; keep_last: but the one built last -- the inputs of it go, it stays"""
        last = self.held.pop() if keep_last else None
        while self.held:
            family, h = self.held.pop()   # (no longer held whatever the free does)
            getattr(self.lib, f"hry_{family}_free")(h)
        if last:
            self.held.append(last)

    def take(self):
        """the handle built last, no longer the chain's to free"""
        return self.held.pop()[1]


def _read_buffers(lib, family: str, h, names, fill, skip_empty: bool = False) -> dict:
    """{name: fill(family, name, rows, width, type, h)} of the named buffers of a handle (hry_<family>_get), in the order of `names`,
    without those the handle does not have (width 0) and, with skip_empty, those without rows"""
    out = {}
    for name in names:
        rows, width, typ = C.c_uint64(), C.c_int(), C.c_int()
        nat.check(getattr(lib, f"hry_{family}_get")(h, name.encode(), None, C.byref(rows), C.byref(width), C.byref(typ)))
        if width.value and (rows.value or not skip_empty):
            out[name] = fill(family, name, rows.value, width.value, typ.value, h)
    return out


def _read_stat(lib, family: str, h, keys=None, extras=None) -> dict:
    """device_ms and uploaded_bytes of a handle (hry_<family>_stat), then `extras`, then the words of its summary under `keys`
    (hry_<family>_summary: 4 words for edges, 6 for the others; keys None: the family has none)"""
    d, up = C.c_double(), C.c_uint64()
    nat.check(getattr(lib, f"hry_{family}_stat")(h, C.byref(d), C.byref(up)))
    out = {"device_ms": d.value, "uploaded_bytes": up.value, **(extras or {})}
    if keys is not None:
        s = (C.c_uint64 * (4 if family == "edges" else 6))()
        nat.check(getattr(lib, f"hry_{family}_summary")(h, s))
        out.update((k, int(s[i])) for i, k in enumerate(keys))
    return out


class Codec:
    """Device context (one HIP device, one stream).  Raises HryError(E_NODEVICE) without a GPU: no CPU fallback."""

    def __init__(self, device: int = 0):
        self.h = C.c_void_p()
        self.device = int(device)
        nat.check(nat.load().hry_ctx_create(device, C.byref(self.h)))

    def close(self):
        if getattr(self, "h", None):
            nat.load().hry_ctx_destroy(self.h)
            self.h = None

    def analysis_check(self, mesh: "Mesh") -> None:
        """Development / tests: the component analysis of `mesh` on the device against the host's, table by table (hry_analysis_check)."""
        nat.check(nat.load().hry_analysis_check(self.h, mesh.h))

    def analysis_tables(self, mesh: "Mesh", where: str = "device") -> dict:
        """Development / tests: the component analysis of `mesh` as numpy arrays by name (hry_analysis_tables), the device's (uploads the
        mesh unless it is resident; with "twin_over", the path its twin matching took) or the host's."""
        if where not in ("device", "host"):
            raise ValueError("where: 'device' or 'host'")
        return _analysis_tables(self.h if where == "device" else None, mesh, where == "device")

    __del__ = close

    def bounds(self, mesh: Mesh):
        nat.check(nat.load().hry_bounds(self.h, mesh.h))

    def requant(self, mesh: Mesh, quants, clear: bool = False):
        """quants: iterable of (list, component or -1, bits) as produced by the reference CLI's -l/-a/-q flags."""
        qs = list(quants)
        arr = (nat.Quant * max(len(qs), 1))(*[nat.Quant(int(l), int(c), int(b)) for l, c, b in qs])
        nat.check(nat.load().hry_requant(self.h, mesh.h, arr, len(qs), int(clear)))

    def upload(self, mesh: Mesh):
        nat.check(nat.load().hry_mesh_upload(self.h, mesh.h))

    def write_hry(self, mesh: Mesh, profile: int = PROFILE_COMPAT, chunk_syms: int = 0, keep_stages: bool = False, flags: int = 0, as_buffer: bool = False,
                  return_order: bool = False):
        """as_buffer: return the library's buffer as it is (nat.NativeBuffer: what a C caller of hry_encode holds) instead of bytes.
        return_order: return (data, Order) -- the numbering maps between `mesh` and what read_hry(data) gives (HRY_FLAG_ORDER)"""
        o = nat.Opts(profile, chunk_syms, int(keep_stages), flags | (FLAG_ORDER if return_order else 0), 0, 0)
        p, n = C.c_void_p(), C.c_size_t()
        nat.check(nat.load().hry_encode(self.h, mesh.h, C.byref(o), C.byref(p), C.byref(n)))
        data = nat.take(p, n.value, as_buffer)
        return (data, self.take_order(mesh)) if return_order else data

    def take_order(self, mesh: Mesh) -> "Order":
        """the numbering maps of the write_hry(mesh, flags=FLAG_ORDER) that was the last call on this codec (hry_order_take)"""
        h = C.c_void_p()
        nat.check(nat.load().hry_order_take(self.h, mesh.h, C.byref(h)))
        return Order(self, h, mesh.nlists if mesh.general else 0)

    def read_hry(self, data: bytes, keep_stages: bool = False, shard=(0, 0), partial: bool = False) -> Mesh:
        """shard = (index, count): of a sharded container decode only the segments i with i % count == index.
        partial: accept a sharded container that does not hold the whole mesh (one rank's own part): the result is a partial mesh."""
        o = nat.Opts(0, 0, int(keep_stages), FLAG_PARTIAL if partial else 0, int(shard[0]), int(shard[1]))
        h = C.c_void_p()
        nat.check(nat.load().hry_decode(self.h, data, len(data), C.byref(o), C.byref(h)))
        return Mesh(h)

    # ---- render-ready device buffers (include/harry_amd.h: hry_render_build)
    RENDER_FIXED = ("indices", "tri_face", "vertex_source", "corner_source", "face_region")
    _RENDER_NP = {0: np.float32, 4: np.uint32, 6: np.uint16}

    RENDER_VERTEX_NORMALS, RENDER_FACE_NORMALS, RENDER_ANGLE_WEIGHTED = 1, 2, 4
    RENDER_NORMALS = ("normals", "face_normals")

    @classmethod
    def _render_flags(cls, normals, face_normals) -> int:
        if normals not in (None, "area", "angle"):
            raise ValueError('normals is one of None, "area", "angle"')
        flags = 0 if normals is None else cls.RENDER_VERTEX_NORMALS | (cls.RENDER_ANGLE_WEIGHTED if normals == "angle" else 0)
        return flags | (cls.RENDER_FACE_NORMALS if face_normals else 0)

    def _render(self, mesh: Mesh, fill, flags: int = 0) -> dict:
        """build, hand every buffer with rows to fill(family, name, rows, width, type, handle), free the handle"""
        with _Chain(self, mesh) as chain:
            r = chain.build("render", flags, entry="hry_render_build_ex") if flags else chain.build("render")
            L = chain.lib
            names = self.RENDER_FIXED + tuple(f"list{l}" for l in range(mesh.nlists)) + (self.RENDER_NORMALS if flags else ())
            out = _read_buffers(L, "render", r, names, fill, skip_empty=True)
            self._render_stat = _read_stat(L, "render", r, extras={"nverts": L.hry_render_nverts(r), "ntris": L.hry_render_ntris(r)})
            return out

    def render_numpy(self, mesh: Mesh, normals=None, face_normals: bool = False) -> dict:
        """the mesh as render-ready buffers (hry_render_build), copied to host arrays: indices u32 [T, 3], tri_face u32 [T],
        vertex_source u32 [U], corner_source u32 [U] (unwelded meshes), face_region u16 [nf] (general bindings), list<l> f32 [rows, ncomp].
        normals "area" / "angle": also normals f32 [U, 3], computed on the device from the positions (hry_render_build_ex), weighted
        by face area / corner angle; face_normals: also face_normals f32 [nf, 3]"""
        return self._render(mesh, self._fill_numpy, self._render_flags(normals, face_normals))

    def render(self, mesh: Mesh, normals=None, face_normals: bool = False) -> dict:
        """the same buffers as torch tensors on this codec's device, copied device to device: indices / tri_face / vertex_source /
        corner_source int32, face_region int16, list<l> / normals / face_normals float32.  They stay valid after close()."""
        if max(mesh.nv, mesh.ne, mesh.ntri) >= 2 ** 31:   # (every u32 value is below one of them: U <= max(nv, ne))
            raise HryError(nat.E_ARG, "vertex, corner or triangle numbers of this mesh do not fit int32 tensors")
        return self._render(mesh, self._torch_fill(), self._render_flags(normals, face_normals))

    # ---- the builds behind a render build: edges, shells, orient (include/harry_amd.h: hry_edges_build, hry_shells_build, hry_orient_build)
    def _topology(self, mesh: Mesh, family: str, flags: int, names, summary, fill) -> dict:
        """the chain of builds that ends in `family` -- render, edges, then shells or orient from both --; its inputs are freed, then
        every named buffer the last handle has goes to fill(family, name, rows, width, type, handle) and its stat and summary (keys:
        `summary`) into self._<family>_stat"""
        with _Chain(self, mesh) as chain:
            r = chain.build("render")
            e = chain.build("edges", r, flags if family == "edges" else 0)
            h = e if family == "edges" else chain.build(family, r, e, flags)
            chain.free(keep_last=True)
            out = _read_buffers(chain.lib, family, h, names, fill)
            setattr(self, f"_{family}_stat", _read_stat(chain.lib, family, h, summary))
            return out

    def _fill_numpy(self, family, name, rows, width, typ, h):
        """the fill that copies into a host array: a row per row, [rows] where a row is one value (a render build's list<l>: [rows, 1])"""
        a = np.empty((rows, width) if width > 1 or name.startswith("list") else (rows,), self._RENDER_NP[typ])
        if rows:
            nat.check(getattr(nat.load(), f"hry_{family}_copy")(self.h, h, name.encode(), a.ctypes.data, 0))
        return a

    def _torch_fill(self):
        """the fill that copies device to device into tensors on this codec's device, shaped as _fill_numpy's arrays: int32 (NO_ELEMENT
        reads -1), int16 and float32"""
        import torch   # only here: the rest of the package does not need torch
        dev = torch.device("cuda", self.device)
        dtypes = {0: torch.float32, 4: torch.int32, 6: torch.int16}
        torch.cuda.current_stream(dev).synchronize()   # (memory torch hands out may still be in use by its own stream)

        def fill(family, name, rows, width, typ, h):
            t = torch.empty((rows, width) if width > 1 or name.startswith("list") else (rows,), dtype=dtypes[typ], device=dev)
            if rows:
                nat.check(getattr(nat.load(), f"hry_{family}_copy")(self.h, h, name.encode(), t.data_ptr(), 1))
            return t
        return fill

    def _fill_torch(self, mesh: Mesh):
        """_torch_fill for the builds behind a render build, whose buffers also number the triangles' sides"""
        if max(mesh.nv, mesh.ne, 3 * mesh.ntri) >= 2 ** 31:   # (every u32 value but NO_ELEMENT is below one of them)
            raise HryError(nat.E_ARG, "vertex, corner or side numbers of this mesh do not fit int32 tensors")
        return self._torch_fill()

    # ---- edges and adjacency of a render build (include/harry_amd.h: hry_edges_build)
    EDGES_FIXED = ("edges", "tri_edges", "edge_offsets", "edge_sides", "tri_neighbours")
    EDGES_GEOMETRY = ("edge_length", "edge_cot", "edge_cos")
    EDGES_SUMMARY = ("edges", "boundary", "manifold", "nonmanifold")

    def _edges(self, mesh: Mesh, fill, geometry: bool) -> dict:
        return self._topology(mesh, "edges", nat.EDGES_GEOMETRY if geometry else 0, self.EDGES_FIXED + (self.EDGES_GEOMETRY if geometry else ()),
                              self.EDGES_SUMMARY, fill)

    def edges_numpy(self, mesh: Mesh, geometry: bool = False) -> dict:
        """unique edges and adjacency of the mesh's render build (hry_edges_build), copied to host arrays: edges u32 [E, 2], tri_edges
        u32 [T, 3], edge_offsets u32 [E + 1], edge_sides u32 [3 T], tri_neighbours u32 [T, 3] (NO_ELEMENT: none); geometry: also
        edge_length, edge_cot, edge_cos f32 [E] (edge_cos 2.0: the edge does not join two triangles with normals)"""
        return self._edges(mesh, self._fill_numpy, geometry)

    def edges(self, mesh: Mesh, geometry: bool = False) -> dict:
        """the same buffers as torch tensors on this codec's device, copied device to device: int32 (NO_ELEMENT reads -1) and float32"""
        return self._edges(mesh, self._fill_torch(mesh), geometry)

    def edges_stat(self) -> dict:
        """of the last edges / edges_numpy: device_ms (the kernels), uploaded_bytes (0), and hry_edges_summary's counts: edges (E),
        boundary (one side), manifold (two), nonmanifold (more)"""
        return dict(getattr(self, "_edges_stat", {}))

    # ---- shells of a render build (include/harry_amd.h: hry_shells_build)
    SHELLS_FIXED = ("tri_shell", "face_shell", "edge_shell", "shell_first", "shell_counts")
    SHELLS_GEOMETRY = ("shell_measures",)
    SHELLS_SUMMARY = ("shells", "closed", "nonmanifold", "misoriented", "loops", "largest")

    def _shells(self, mesh: Mesh, fill, geometry: bool) -> dict:
        return self._topology(mesh, "shells", nat.SHELLS_GEOMETRY if geometry else 0, self.SHELLS_FIXED + (self.SHELLS_GEOMETRY if geometry else ()),
                              self.SHELLS_SUMMARY, fill)

    def shells_numpy(self, mesh: Mesh, geometry: bool = False) -> dict:
        """the shells of the mesh's render build (hry_shells_build), copied to host arrays: tri_shell u32 [T], face_shell u32 [nf],
        edge_shell u32 [E], shell_first u32 [S], shell_counts u32 [S, 8] (triangles, faces, vertices, edges, boundary, nonmanifold,
        misoriented, loops); geometry: also shell_measures f32 [S, 8] (area, signed volume, min x y z, max x y z)"""
        return self._shells(mesh, self._fill_numpy, geometry)

    def shells(self, mesh: Mesh, geometry: bool = False) -> dict:
        """the same buffers as torch tensors on this codec's device, copied device to device: int32 (NO_ELEMENT reads -1) and float32"""
        return self._shells(mesh, self._fill_torch(mesh), geometry)

    def shells_stat(self) -> dict:
        """of the last shells / shells_numpy: device_ms (the kernels), uploaded_bytes (0), and hry_shells_summary's counts: shells (S),
        closed, nonmanifold, misoriented (shells), loops (over all shells), largest (triangles of the largest shell)"""
        return dict(getattr(self, "_shells_stat", {}))

    # ---- a consistent winding per patch of a render build (include/harry_amd.h: hry_orient_build)
    ORIENT_FIXED = ("tri_patch", "tri_flip", "face_flip", "oriented_indices", "patch_first", "patch_counts")
    ORIENT_OUTWARD = ("patch_measures",)
    ORIENT_SUMMARY = ("patches", "orientable", "flipped", "inverted", "against", "remaining")

    def _orient(self, mesh: Mesh, fill, majority: bool, outward: bool) -> dict:
        flags = (nat.ORIENT_MAJORITY if majority else 0) | (nat.ORIENT_OUTWARD if outward else 0)
        return self._topology(mesh, "orient", flags, self.ORIENT_FIXED + (self.ORIENT_OUTWARD if outward else ()), self.ORIENT_SUMMARY, fill)

    def orient_numpy(self, mesh: Mesh, majority: bool = False, outward: bool = False) -> dict:
        """which triangles of the mesh's render build to turn for a consistent winding per patch (hry_orient_build), copied to host
        arrays: tri_patch u32 [T], tri_flip u32 [T], face_flip u32 [nf], oriented_indices u32 [T, 3], patch_first u32 [P], patch_counts
        u32 [P, 8] (triangles, faces, flipped, flipped_faces, against, open, orientable, inverted); majority: the smaller side of every
        patch is flipped; outward: closed patches enclose a positive volume, and patch_measures f32 [P, 8] (area, signed volume, min x y
        z, max x y z).  mesh.flip_faces(face_flip) is the oriented mesh"""
        return self._orient(mesh, self._fill_numpy, majority, outward)

    def orient(self, mesh: Mesh, majority: bool = False, outward: bool = False) -> dict:
        """the same buffers as torch tensors on this codec's device, copied device to device: int32 and float32"""
        return self._orient(mesh, self._fill_torch(mesh), majority, outward)

    def orient_stat(self) -> dict:
        """of the last orient / orient_numpy: device_ms (the kernels), uploaded_bytes (0), and hry_orient_summary's counts: patches (P),
        orientable (patches), flipped (triangles), inverted (patches), against (edges), remaining (against edges in patches that cannot
        be oriented)"""
        return dict(getattr(self, "_orient_stat", {}))

    # ---- tangent frames of a render build (include/harry_amd.h: hry_tangents_build)
    TANGENTS_SUMMARY = ("framed", "unframed", "mirrored", "mixed", "degenerate")

    def _tangents(self, mesh: Mesh, normals, weights, bitangents: bool, fill) -> dict:
        """the render build with the normals asked for, the tangents build behind it; "tangents", "bitangents" and the render's
        "indices" and "vertex_source" go to fill(family, name, rows, width, type, handle); both handles are freed whatever happens"""
        if normals not in ("area", "angle", "stored"):
            raise ValueError('normals is one of "area", "angle", "stored"')
        if weights not in ("area", "angle"):
            raise ValueError('weights is one of "area", "angle"')
        stored = normals == "stored"
        flags = ((nat.TANGENTS_ANGLE_WEIGHTED if weights == "angle" else 0) | (nat.TANGENTS_STORED_NORMALS if stored else 0) |
                 (nat.TANGENTS_BITANGENTS if bitangents else 0))
        with _Chain(self, mesh) as chain:
            r = chain.build("render", 0 if stored else self._render_flags(normals, False), entry="hry_render_build_ex")
            t = chain.build("tangents", r, flags)
            L = chain.lib
            out = {**_read_buffers(L, "tangents", t, ("tangents", "bitangents"), fill), **_read_buffers(L, "render", r, ("indices", "vertex_source"), fill)}
            self._tangents_stat = _read_stat(L, "tangents", t, self.TANGENTS_SUMMARY, self._render_times(L, r))
            return out

    @staticmethod
    def _render_times(lib, r) -> dict:
        """hry_render_stat of the render build another build lies behind, under that build's keys"""
        s = _read_stat(lib, "render", r)
        return {"render_device_ms": s["device_ms"], "render_uploaded_bytes": s["uploaded_bytes"]}

    def tangents_numpy(self, mesh: Mesh, normals: str = "area", weights: str = "area", bitangents: bool = False) -> dict:
        """a tangent frame per output vertex of the mesh's render build (hry_tangents_build), copied to host arrays: tangents f32 [U, 4]
        (unit tangent, handedness +1 / -1; a zero row: no frame), bitangents f32 [U, 3] where asked for, and the render build's
        indices u32 [T, 3] and vertex_source u32 [U] they go with.  normals: "area" / "angle": computed on the device with those
        weights, "stored": the file's (nx ny nz, OBJ vn); weights: "area": uv-area weights, "angle": unit directions weighted by the
        corner's angle"""
        return self._tangents(mesh, normals, weights, bitangents, self._fill_numpy)

    def tangents(self, mesh: Mesh, normals: str = "area", weights: str = "area", bitangents: bool = False) -> dict:
        """the same buffers as torch tensors on this codec's device, copied device to device: float32 and int32"""
        return self._tangents(mesh, normals, weights, bitangents, self._fill_torch(mesh))

    def tangents_stat(self) -> dict:
        """of the last tangents / tangents_numpy: device_ms (the kernels), uploaded_bytes (0), and hry_tangents_summary's counts: framed,
        unframed (vertices with a zero row), mirrored (w = -1), mixed (both signs of the uv determinant meet) vertices, degenerate
        (uv-degenerate triangles); render_device_ms / render_uploaded_bytes: hry_render_stat of the render build it was built behind"""
        return dict(getattr(self, "_tangents_stat", {}))

    # ---- hard edges and split normals of a render build (include/harry_amd.h: hry_creases_build)
    CREASES_BUFFERS = ("indices", "render_vertex", "vertex_source", "normals", "slot_group", "edge_class")
    CREASES_SUMMARY = ("vertices", "groups", "smooth", "sharp", "split", "other")

    def _creases(self, mesh: Mesh, angle, cos_limit, weights, fill, gather) -> dict:
        """the render build, its edges build with geometry, the creases build behind both; the creases' buffers go to fill(family, name,
        rows, width, type, handle), and "positions" is gather(the render's position list filled the same way, its first position
        component, render_vertex); all three handles are freed whatever happens"""
        if weights not in ("area", "angle"):
            raise ValueError('weights is one of "area", "angle"')
        limit = float(math.cos(math.radians(angle)) if cos_limit is None else cos_limit)
        with _Chain(self, mesh) as chain:
            r = chain.build("render")
            e = chain.build("edges", r, nat.EDGES_GEOMETRY)
            c = chain.build("creases", r, e, limit, nat.CREASES_ANGLE_WEIGHTED if weights == "angle" else 0)
            L = chain.lib
            out = _read_buffers(L, "creases", c, self.CREASES_BUFFERS, fill)
            # the position list as the library chooses it (render.cpp: position_list): list 1, or the one vertex list with positions
            pl = [l for l in range(mesh.nlists) if mesh.list_target(l) == 1 and L.hry_list_interp_ncomp(mesh.h, l, 0) >= 3][0]
            rows = _read_buffers(L, "render", r, (f"list{pl}",), fill)[f"list{pl}"]
            out["positions"] = gather(rows, L.hry_list_interp_offset(mesh.h, pl, 0), out["render_vertex"])
            extras = {"edges_device_ms": _read_stat(L, "edges", e)["device_ms"], **self._render_times(L, r), "cos_limit": limit}
            self._creases_stat = _read_stat(L, "creases", c, self.CREASES_SUMMARY, extras)
            return out

    def creases_numpy(self, mesh: Mesh, angle: float = 30.0, cos_limit=None, weights: str = "area") -> dict:
        """the mesh's render build with its vertices split along hard edges (hry_creases_build), copied to host arrays: indices u32
        [T, 3], render_vertex u32 [W], vertex_source u32 [W], normals f32 [W, 3], slot_group u32 [T, 3], edge_class u32 [E]
        (nat.CREASE_*), and positions f32 [W, 3], the render build's position rows gathered by render_vertex.  angle: the crease angle
        in degrees, an edge that folds more sharply is hard -- the limit is math.cos(math.radians(angle)); cos_limit: the limit
        itself, exact at equality (<= -1: all smooth, > 1: flat shading); weights: "area": the triangles' areas, "angle": the
        corners' angles"""
        return self._creases(mesh, angle, cos_limit, weights, self._fill_numpy,
                             lambda rows, at, rv: np.ascontiguousarray(rows.reshape(len(rows), -1)[rv.astype(np.int64), at:at + 3]))

    def creases(self, mesh: Mesh, angle: float = 30.0, cos_limit=None, weights: str = "area") -> dict:
        """the same buffers as torch tensors on this codec's device, copied device to device: float32 and int32"""
        return self._creases(mesh, angle, cos_limit, weights, self._fill_torch(mesh),
                             lambda rows, at, rv: rows.reshape(len(rows), -1)[rv.long(), at:at + 3].contiguous())

    def creases_stat(self) -> dict:
        """of the last creases / creases_numpy: device_ms (the kernels), uploaded_bytes (0), cos_limit (the limit used), and
        hry_creases_summary's counts: vertices (W), groups (G), smooth, sharp (edges), split (decoded vertices with more than one
        group), other (boundary, non-manifold, misoriented and degenerate edges); edges_device_ms: of the edges build before it;
        render_device_ms / render_uploaded_bytes: hry_render_stat of the render build before both"""
        return dict(getattr(self, "_creases_stat", {}))

    # ---- vertex areas and curvatures of a render build (include/harry_amd.h: hry_curvature_build)
    CURVATURE_BUFFERS = ("vertex_class", "vertex_area", "angle_defect", "gaussian", "mean_normal", "mean")
    CURVATURE_SUMMARY = ("vertices", "interior", "boundary", "irregular", "isolated", "degenerate")
    CURVATURE_TOTALS = ("area", "defect", "mean_integral")

    def _curvature(self, mesh: Mesh, fill) -> dict:
        """the render build, its edges build, the curvature build behind both; the curvature's buffers go to fill(family, name, rows,
        width, type, handle); all three handles are freed whatever happens"""
        with _Chain(self, mesh) as chain:
            r = chain.build("render")
            e = chain.build("edges", r, 0)
            c = chain.build("curvature", r, e, 0)
            L = chain.lib
            out = _read_buffers(L, "curvature", c, self.CURVATURE_BUFFERS, fill)
            t = (C.c_double * 3)()
            nat.check(L.hry_curvature_totals(c, t))
            self._curvature_stat = {**_read_stat(L, "curvature", c, self.CURVATURE_SUMMARY, {"edges_device_ms": _read_stat(L, "edges", e)["device_ms"]}),
                                    **{k: float(t[i]) for i, k in enumerate(self.CURVATURE_TOTALS)}}
            return out

    def curvature_numpy(self, mesh: Mesh, principal: bool = False) -> dict:
        """the discrete curvatures of the mesh's render build (hry_curvature_build), copied to host arrays of U rows, row u the value of
        decoded vertex vertex_source[u]: vertex_class u32 [U] (nat.VERTEX_*: 0 isolated, 1 interior, 2 boundary, 3 irregular, 8 or-ed
        in: no usable area), vertex_area f32 [U] (mixed Voronoi area), angle_defect f32 [U], gaussian f32 [U], mean_normal f32 [U, 3]
        (the mean curvature vector H n), mean f32 [U] (positive where the surface is convex towards its normal).
        principal: also "principal" f32 [U, 2] = (H + r, H - r) with r = sqrt(max(H * H - K, 0)), computed here in float32 from the
        returned mean and gaussian.  It is no device buffer and has no bit contract: at umbilic points (a sphere) H * H - K cancels
        and r is ill-conditioned, so a promise about its bits would not be an honest one"""
        out = self._curvature(mesh, self._fill_numpy)
        if principal:
            h, k = out["mean"], out["gaussian"]
            r = np.sqrt(np.maximum(h * h - k, np.float32(0)))
            out["principal"] = np.stack([h + r, h - r], axis=1).astype(np.float32)
        return out

    def curvature(self, mesh: Mesh, principal: bool = False) -> dict:
        """the same buffers as torch tensors on this codec's device, copied device to device: float32 and int32; "principal" in plain
        torch, float32, with the same caveat"""
        out = self._curvature(mesh, self._fill_torch(mesh))
        if principal:
            import torch   # only here: the rest of the package does not need torch
            h, k = out["mean"], out["gaussian"]
            r = torch.sqrt(torch.clamp(h * h - k, min=0))
            out["principal"] = torch.stack([h + r, h - r], dim=1)
        return out

    def curvature_stat(self) -> dict:
        """of the last curvature / curvature_numpy: device_ms (the kernels), uploaded_bytes (0), edges_device_ms (of the edges build
        before it), hry_curvature_summary's counts over decoded vertices: vertices (D), interior, boundary, irregular, isolated,
        degenerate (bit 8: no usable area), and hry_curvature_totals: area (the sum of the vertex areas), defect (of the angle defects:
        2 pi times the Euler characteristic of a closed manifold mesh), mean_integral (of mean curvature times area)"""
        return dict(getattr(self, "_curvature_stat", {}))

    # ---- ray queries on a render build (include/harry_amd.h: hry_bvh_build, hry_bvh_cast)
    def bvh(self, mesh: Mesh) -> "Bvh":
        """a bounding-volume hierarchy over the triangles of the mesh's render build, built on the device (hry_bvh_build): an owning
        object like Order, valid whatever the codec does later, until close().  The render build is freed before this returns"""
        with _Chain(self, mesh) as chain:
            chain.build("bvh", chain.build("render"), 0)
            b = chain.take()
        out = Bvh(self, b)
        self._bvh_stat = out.stat()
        return out

    def bvh_stat(self) -> dict:
        """of the last bvh(): device_ms (the kernels), uploaded_bytes (0) and hry_bvh_summary's counts: triangles (T), leaves (L: the
        live triangles), dead (T - L: a position that is not finite), distinct_codes, depth (internal nodes from the root to the
        deepest leaf, at most 62)"""
        return dict(getattr(self, "_bvh_stat", {}))

    # ---- self-intersections (include/harry_amd.h: hry_intersections_build)
    def intersections(self, mesh: Mesh) -> "Intersections":
        """the pairs of the mesh's triangles that pass through each other (Bvh.intersections): the render build and the hierarchy
        over it are built and freed here, the result stays until close()"""
        b = self.bvh(mesh)
        try:
            return b.intersections()
        finally:
            b.close()

    # ---- mesh-to-mesh deviation (include/harry_amd.h: hry_bvh_nearest)
    def position_rows(self, mesh: Mesh) -> np.ndarray:
        """the float rows [U, 3] of the positions of the mesh's render build (dequantised, one row per output vertex): a view into
        the rows of its position list"""
        L = nat.load()
        rn = self.render_numpy(mesh)
        (pl,) = [l for l in range(mesh.nlists) if mesh.list_target(l) == 1 and L.hry_list_interp_ncomp(mesh.h, l, 0) >= 3]
        at = L.hry_list_interp_offset(mesh.h, pl, 0)
        return rn[f"list{pl}"][:, at:at + 3]

    def deviation(self, a: Mesh, b: Mesh) -> dict:
        """the Metro-style deviation of two surfaces, sampled at their vertices: "forward" -- the position rows of a's render build
        against the closest points of b's triangles --, "backward" -- b's rows against a's triangles --, each {"points", "answered"
        (rows with finite positions, where the other mesh has a live triangle), "max", "rms"}, and "hausdorff", the larger max.
        The squared distances are hry_bvh_nearest's; the square roots are taken here, rms = sqrt(the sum of d2 in index order /
        answered), in double"""
        def one_way(points, surface: "Bvh") -> dict:
            d2 = surface.nearest_numpy(points)["d2"] if len(points) else np.zeros(0)
            answered = np.isfinite(d2)
            total = 0.0
            for x in d2[answered].tolist():
                total += x
            k = int(answered.sum())
            return {"points": len(points), "answered": k, "max": math.sqrt(surface.max_d2) if k else 0.0, "rms": math.sqrt(total / k) if k else 0.0}

        pa, pb = self.position_rows(a), self.position_rows(b)
        ba = self.bvh(a)
        try:
            bb = self.bvh(b)
            try:
                out = {"forward": one_way(pa, bb), "backward": one_way(pb, ba)}
            finally:
                bb.close()
        finally:
            ba.close()
        out["hausdorff"] = max(out["forward"]["max"], out["backward"]["max"])
        return out

    # ---- meshes from device buffers (include/harry_amd.h: hry_mesh_from_device)
    def mesh_from_tensors(self, indices, vertex, faces=None, degrees=None, weld: bool = False, return_remap: bool = False):
        """A mesh from torch tensors on this codec's device, equal to Mesh.from_arrays of the same values and resident here (the
        encoder uploads nothing for it).  indices: int32 / int64, [T, 3] (every face a triangle) or 1-D with degrees (uint8 [nf]);
        vertex / faces: [(names, tensor)], names one per column ("x y z"), tensor [n] for one name or [n, k] for k names, passed
        with its own strides (views need no copy).  weld: vertices whose records are equal byte for byte become one, numbered in
        order of first occurrence; return_remap: also the output vertex of every input row (int32 [nv] on this device)."""
        import torch   # only here: the rest of the package does not need torch
        dev = torch.device("cuda", self.device)
        types = {torch.float32: 0, torch.float64: 1, torch.int64: 3, torch.int32: 5, torch.int16: 7, torch.uint8: 8, torch.int8: 9}
        for name, t in (("uint64", 2), ("uint32", 4), ("uint16", 6)):
            if hasattr(torch, name):
                types[getattr(torch, name)] = t

        def refuse(msg):
            return HryError(nat.E_ARG, msg)

        def tensor(t, what):
            if not isinstance(t, torch.Tensor) or t.device != dev:
                raise refuse(f"{what}: not a tensor on {dev}")
            return t

        def columns(spec, what):
            cols, rows = [], None
            for names, t in spec or ():
                tensor(t, what)
                names = names.split() if isinstance(names, str) else list(names)
                if t.dtype not in types:
                    raise refuse(f"{what} {' '.join(names)}: unsupported dtype {t.dtype}")
                if not ((t.dim() == 1 and len(names) == 1) or (t.dim() == 2 and t.shape[1] == len(names))):
                    raise refuse(f"{what} {' '.join(names)}: shape {tuple(t.shape)} does not fit {len(names)} names")
                if rows is not None and t.shape[0] != rows:
                    raise refuse(f"{what} {' '.join(names)}: {t.shape[0]} rows, the others have {rows}")
                rows, item = t.shape[0], t.element_size()
                for j, name in enumerate(names):
                    off = j * t.stride(1) * item if t.dim() == 2 else 0
                    cols.append(nat.DevColumn(t.data_ptr() + off, t.stride(0) * item, name.encode(), types[t.dtype]))
            return cols, rows or 0

        tensor(indices, "indices")
        if indices.dtype not in (torch.int32, torch.int64):
            raise refuse(f"indices: dtype {indices.dtype} (int32 or int64)")
        if degrees is None:
            if indices.dim() != 2 or indices.shape[1] != 3:
                raise refuse("indices: [T, 3] without degrees")
            nf = indices.shape[0]
        else:
            tensor(degrees, "degrees")
            if degrees.dtype != torch.uint8 or degrees.dim() != 1 or indices.dim() != 1:
                raise refuse("degrees: uint8 [nf] with 1-D indices")
            degrees = degrees.contiguous()
            nf = degrees.shape[0]
        indices = indices.contiguous()
        vcols, nv = columns(vertex, "vertex")
        fcols, nff = columns(faces, "face")
        if fcols and nff != nf:
            raise refuse(f"face columns: {nff} rows for {nf} faces")
        if max(nv, nf, indices.numel()) >= 2 ** 32:
            raise refuse("more than 2^32 - 1 vertices, faces or indices")
        remap = torch.empty(nv, dtype=torch.int32, device=dev) if return_remap else None
        torch.cuda.current_stream(dev).synchronize()   # (the tensors may still be being written by torch's stream)
        h = C.c_void_p()
        va = (nat.DevColumn * max(len(vcols), 1))(*vcols)
        fa = (nat.DevColumn * max(len(fcols), 1))(*fcols)
        nat.check(nat.load().hry_mesh_from_device(
            self.h, nv, va, len(vcols), nf, degrees.data_ptr() if degrees is not None else None, indices.data_ptr() if indices.numel() else None,
            4 if indices.dtype == torch.int32 else 3, indices.numel(), fa, len(fcols), nat.INGEST_WELD if weld else 0,
            remap.data_ptr() if remap is not None and nv else None, C.byref(h)))
        mesh = Mesh(h)
        return (mesh, remap) if return_remap else mesh

    def corner_mesh_from_tensors(self, positions, pos_idx, uv=None, uv_idx=None, normals=None, normal_idx=None, degrees=None,
                                 materials=None, weld: bool = False, return_remap: bool = False):
        """hry_mesh_from_device_corners: the mesh Mesh.from_obj builds from the text of the same arrays, from tensors on this codec's
        device and resident here.  positions [n, 3 | 4 | 6 | 7 | 8], uv [n, 2 | 3], normals [n, 3]: float32, passed with their own
        strides.  pos_idx / uv_idx / normal_idx: the row every corner names, int32 [T, 3] or 1-D int32 / int64 with degrees (uint8
        [nf]); uv_idx / normal_idx None: pos_idx (the layout Codec.render returns).  materials: int16 (or uint16) [nf], one region
        per distinct value in order of first occurrence.  weld: every list on its own, rows equal byte for byte become one record;
        return_remap: also (pos, uv, normal) int32 tensors with the output record of every input row, None for absent lists."""
        import torch   # only here: the rest of the package does not need torch
        dev = torch.device("cuda", self.device)

        def refuse(msg):
            return HryError(nat.E_ARG, msg)

        def tensor(t, what):
            if not isinstance(t, torch.Tensor) or t.device != dev:
                raise refuse(f"{what}: not a tensor on {dev}")
            return t

        tensor(pos_idx, "pos_idx")
        if pos_idx.dtype not in (torch.int32, torch.int64):
            raise refuse(f"pos_idx: dtype {pos_idx.dtype} (int32 or int64)")
        if degrees is None:
            if pos_idx.dim() != 2 or pos_idx.shape[1] != 3:
                raise refuse("pos_idx: [T, 3] without degrees")
            nf = pos_idx.shape[0]
        else:
            tensor(degrees, "degrees")
            if degrees.dtype != torch.uint8 or degrees.dim() != 1 or pos_idx.dim() != 1:
                raise refuse("degrees: uint8 [nf] with 1-D indices")
            degrees = degrees.contiguous()
            nf = degrees.shape[0]
        pos_idx = pos_idx.contiguous()
        keep, rows, remaps = [], [], []
        for what, t, idx in (("positions", positions, pos_idx), ("uv", uv, uv_idx), ("normals", normals, normal_idx)):
            if t is None:
                if idx is not None and what != "positions":
                    raise refuse(f"{what}: indices without rows")
                rows.append(None)
                remaps.append(None)
                continue
            tensor(t, what)
            if t.dtype != torch.float32 or t.dim() != 2:
                raise refuse(f"{what}: float32 [n, k], not {t.dtype} {tuple(t.shape)}")
            if idx is None:
                idx = pos_idx
            elif idx is not pos_idx:
                tensor(idx, what + " indices")
                if idx.dtype != pos_idx.dtype or idx.shape != pos_idx.shape:
                    raise refuse(f"{what} indices: {idx.dtype} {tuple(idx.shape)}, pos_idx is {pos_idx.dtype} {tuple(pos_idx.shape)}")
                idx = idx.contiguous()
            if t.shape[0] >= 2 ** 32:
                raise refuse("more than 2^32 - 1 rows")
            cols = (nat.DevColumn * t.shape[1])(*[nat.DevColumn(t.data_ptr() + j * t.stride(1) * 4, t.stride(0) * 4, None, 0) for j in range(t.shape[1])])
            remap = torch.empty(t.shape[0], dtype=torch.int32, device=dev) if return_remap else None
            keep += [cols, idx]
            rows.append(nat.DevRows(cols, t.shape[1], t.shape[0], idx.data_ptr() if idx.numel() else None))
            remaps.append(remap)
        if materials is not None:
            tensor(materials, "materials")
            if materials.dtype not in (torch.int16, getattr(torch, "uint16", torch.int16)) or materials.dim() != 1 or materials.shape[0] != nf:
                raise refuse(f"materials: int16 [{nf}], not {materials.dtype} {tuple(materials.shape)}")
            materials = materials.contiguous()
        if max(nf, pos_idx.numel()) >= 2 ** 32:
            raise refuse("more than 2^32 - 1 faces or indices")
        torch.cuda.current_stream(dev).synchronize()   # (the tensors may still be being written by torch's stream)
        h = C.c_void_p()
        out_remap = (C.c_void_p * 3)(*[r.data_ptr() if r is not None and r.numel() else None for r in remaps])
        nat.check(nat.load().hry_mesh_from_device_corners(
            self.h, *[C.byref(r) if r is not None else None for r in rows], nf, degrees.data_ptr() if degrees is not None else None,
            4 if pos_idx.dtype == torch.int32 else 3, pos_idx.numel(), materials.data_ptr() if materials is not None and nf else None,
            nat.INGEST_WELD if weld else 0, out_remap if return_remap else None, C.byref(h)))
        mesh = Mesh(h)
        return (mesh, tuple(remaps)) if return_remap else mesh

    def distortion(self, src: Mesh, other: Mesh, order: "Order | None" = None, rows: bool = False) -> "Distortion":
        """hry_distortion_build: the error of `other` against `src`, component by component, on the device.  order: the numbering
        maps of the encode that relates them (write_hry(..., return_order=True)), None: row i against row i.  rows: also one error
        value per row of every compared list ("error<l>", float32 in HBM)"""
        return self.distortion_ex(src, other, order, rows)

    def distortion_ex(self, src: Mesh, other: Mesh, order: "Order | None" = None, rows: bool = False, normals: bool = False) -> "Distortion":
        """distortion with the build's further flags.  normals: also the angle between each face's normal before and after
        (HRY_DISTORTION_NORMALS: Distortion.normals; with rows the per-face buffer "normal_error")"""
        h = C.c_void_p()
        nat.check(nat.load().hry_distortion_build(self.h, src.h, other.h, order.h if order is not None else None,
                                                  (nat.DISTORTION_ROWS if rows else 0) | (nat.DISTORTION_NORMALS if normals else 0), C.byref(h)))
        return Distortion(self, h)

    def quant_sweep(self, mesh: Mesh, normals: bool = False) -> "QuantSweep":
        """hry_quant_sweep_build(_ex): the error of every quantisation width of every unquantised component of `mesh`, in one pass on
        the device; QuantSweep.choose turns tolerances into the requests for requant.  normals: also the faces' normal deviation at
        every width of the positions (QuantSweep.normals, the "normal_chord" metric)"""
        h = C.c_void_p()
        if normals:
            nat.check(nat.load().hry_quant_sweep_build_ex(self.h, mesh.h, nat.SWEEP_NORMALS, C.byref(h)))
        else:
            nat.check(nat.load().hry_quant_sweep_build(self.h, mesh.h, C.byref(h)))
        return QuantSweep(h)

    def rate_sweep(self, mesh: Mesh) -> "RateSweep":
        """hry_rate_sweep_build: the byte-plane histograms of the residual codes of list 1's components at every quantisation width,
        in one pass over the coding order; RateSweep.choose turns a byte budget into a width.  Walks `mesh` and leaves it resident,
        as write_hry does"""
        h = C.c_void_p()
        nat.check(nat.load().hry_rate_sweep_build(self.h, mesh.h, C.byref(h)))
        return RateSweep(h)

    def resident(self, mesh: Mesh) -> bool:
        """hry_mesh_resident: this context holds the mesh's records and connectivity in HBM (an encode uploads nothing for it)"""
        return bool(nat.load().hry_mesh_resident(self.h, mesh.h))

    def render_stat(self) -> dict:
        """of the last render / render_numpy: device_ms (render kernels), uploaded_bytes (host to device), nverts (U), ntris (T)"""
        return dict(getattr(self, "_render_stat", {}))

    def timing(self) -> dict:
        t = nat.Timing()
        nat.check(nat.load().hry_ctx_timing(self.h, C.byref(t)))
        return t.asdict()

    def stream(self) -> int:
        return nat.load().hry_ctx_stream(self.h) or 0

    def stage(self, name: str, dtype=np.uint8) -> np.ndarray:
        p, n = C.c_void_p(), C.c_size_t()
        nat.check(nat.load().hry_stage_get(self.h, name.encode(), C.byref(p), C.byref(n)))
        return np.frombuffer(nat.take_bytes(p, n.value), dtype=dtype).copy()

    def range_encode_lht(self, lht: np.ndarray) -> bytes:
        lht = np.ascontiguousarray(lht, np.uint64).reshape(-1, 3)
        p, n = C.c_void_p(), C.c_size_t()
        nat.check(nat.load().hry_range_encode_lht(self.h, lht.ctypes.data, len(lht), C.byref(p), C.byref(n)))
        return nat.take_bytes(p, n.value)


def laplacian(edges, weights, n: int):
    """the symmetric n x n torch.sparse_coo_tensor L of an edge list: L[a, b] = L[b, a] = -w for every edge (a, b) with weight w, and
    on the diagonal the row sums of the weights, so that every row of L sums to 0 (edges / edge_cot of Codec.edges: the cotangent
    Laplacian; weights of ones: the graph Laplacian).  Self-edges (a == b) contribute nothing.  Plain torch, coalesced"""
    import torch
    e = edges.to(torch.int64)
    a, b = e[:, 0], e[:, 1]
    w = weights.to(torch.float32)
    w = torch.where(a == b, torch.zeros_like(w), w)
    rows = torch.cat([a, b, a, b])
    cols = torch.cat([b, a, a, b])
    return torch.sparse_coo_tensor(torch.stack([rows, cols]), torch.cat([-w, -w, w, w]), (n, n)).coalesce()


def chord_angle(chord: float) -> float:
    """hry_chord_angle: the angle in radians between two unit normals whose difference has length `chord`: 2 asin(min(chord / 2, 1))"""
    out = C.c_double()
    nat.check(nat.load().hry_chord_angle(float(chord), C.byref(out)))
    return out.value


def angle_chord(radians: float) -> float:
    """hry_angle_chord: 2 sin(radians / 2), the chord a tolerance on the angle between normals is stated in"""
    out = C.c_double()
    nat.check(nat.load().hry_angle_chord(float(radians), C.byref(out)))
    return out.value


def _normal_record(e) -> dict:
    """hry_normal_error as a dict, plus max_angle_deg = the angle of max_chord and rms_angle_deg, DEFINED as the angle of the rms chord,
    chord_angle(sqrt(sum_sq_chord / compared)) -- not the rms of the angles; both 0 when nothing was compared"""
    out = {k: getattr(e, k) for k, _ in e._fields_}
    out["max_angle_deg"] = math.degrees(chord_angle(e.max_chord)) if e.compared else 0.0
    out["rms_angle_deg"] = math.degrees(chord_angle(math.sqrt(e.sum_sq_chord / e.compared))) if e.compared else 0.0
    return out


class _NamedBuffers:
    """A native handle whose buffers lie in HBM and are found by name (hry_<_PREFIX>_get / _copy / _free), rows of one
    component of _NP / _TORCH each.  Order and Distortion say what each accessor gives for them.  _TYPED: the family's get also
    gives a buffer's width and type, as those behind a render build do (Bvh, which reads its buffers with the Codec's fills)"""

    _PREFIX, _NP, _TORCH, _TYPED = "", None, "", False

    def _fn(self, what: str):
        return getattr(nat.load(), f"hry_{self._PREFIX}_{what}")

    def close(self):
        if getattr(self, "h", None):
            self._fn("free")(self.h)
            self.h = None

    __del__ = close

    def _get(self, name: str, dev=None) -> int:
        rows = C.c_uint64()
        nat.check(self._fn("get")(self.h, name.encode(), dev, C.byref(rows), *((None, None) if self._TYPED else ())))
        return rows.value

    def rows(self, name: str) -> int:
        return self._get(name)

    def data_ptr(self, name: str) -> int:
        dev = C.c_void_p()
        self._get(name, C.byref(dev))
        return dev.value or 0

    def numpy(self, name: str) -> np.ndarray:
        a = np.empty(self.rows(name), self._NP)
        nat.check(self._fn("copy")(self.codec.h, self.h, name.encode(), a.ctypes.data, 0))
        return a

    def tensor(self, name: str):
        import torch   # only here: the rest of the package does not need torch
        dev = torch.device("cuda", self.codec.device)
        torch.cuda.current_stream(dev).synchronize()   # (memory torch hands out may still be in use by its own stream)
        t = torch.empty((self.rows(name),), dtype=getattr(torch, self._TORCH), device=dev)
        nat.check(self._fn("copy")(self.codec.h, self.h, name.encode(), t.data_ptr(), 1))
        return t


class Order(_NamedBuffers):
    """The numbering maps of one encode (include/harry_amd.h: hry_order_take): which element of read_hry(write_hry(mesh)) every
    vertex, face, half-edge ("corner") and -- with general bindings -- record of list l ("list<l>") of `mesh` becomes, and the inverses
    ("<name>_inv": source element of every decoded element).  u32 tables in HBM, NO_ELEMENT where an element was never coded (a
    vertex no face names) or a decoded row is filler.  The tables stay valid whatever the codec does later, until close()."""

    KINDS = ("vertex", "face", "corner")
    _PREFIX, _NP, _TORCH = "order", np.uint32, "int32"

    def __init__(self, codec: "Codec", handle, nlists: int = 0):
        self.codec, self.h = codec, handle
        self.names = tuple(n + sfx for n in self.KINDS + tuple(f"list{l}" for l in range(nlists)) for sfx in ("", "_inv"))

    def rows(self, name: str) -> int:
        """rows of a map; 0: there is no such map"""
        return super().rows(name)

    def data_ptr(self, name: str) -> int:
        """device address of a map (u32 [rows]); 0 when absent"""
        return super().data_ptr(name)

    def numpy(self, name: str) -> np.ndarray:
        """a map as a host array (uint32)"""
        return super().numpy(name)

    def tensor(self, name: str):
        """a map as a torch int64 tensor on the codec's device, ready for indexing; NO_ELEMENT becomes -1"""
        import torch   # only here: the rest of the package does not need torch
        t = super().tensor(name)
        w = t.to(torch.int64)
        return torch.where(t == -1, w, w & 0xFFFFFFFF)

    def _apply(self, t, kind: str, direction: int, out):
        import torch   # only here: the rest of the package does not need torch
        dev = torch.device("cuda", self.codec.device)

        def rows_of(x, what):
            if not isinstance(x, torch.Tensor) or x.device != dev or x.dim() < 1:
                raise HryError(nat.E_ARG, f"{what}: a torch tensor on {dev} with at least one dimension")
            if x.shape[0] > 1 and x.dim() > 1 and not x[0].is_contiguous():
                raise HryError(nat.E_ARG, f"{what}: the inner dimensions must be contiguous")
            return x.stride(0) * x.element_size() if x.shape[0] > 1 else max(x[0].numel(), 1) * x.element_size()
        src_stride = rows_of(t, "t")
        if out is None:
            out = torch.empty(t.shape, dtype=t.dtype, device=dev)
        elif out.shape != t.shape or out.dtype != t.dtype:
            raise HryError(nat.E_ARG, "out: the shape and dtype of t")
        dst_stride = rows_of(out, "out")
        row_bytes = (t[0].numel() if t.shape[0] else 1) * t.element_size()
        if t.shape[0] == 0 and self.rows(kind) == 0:
            return out
        torch.cuda.current_stream(dev).synchronize()   # (the caller's tensors may still be written by torch's own stream)
        nat.check(nat.load().hry_order_apply(self.codec.h, self.h, kind.encode(), direction, t.data_ptr(), src_stride, out.data_ptr(), dst_stride,
                                             row_bytes, t.shape[0]))
        return out

    def to_decoded(self, t, kind: str = "vertex", out=None):
        """rows in source order -> rows in decoded order: result[j] = t[kind_inv[j]], zero bytes where the decoded row is filler.
        t: a torch tensor on the codec's device of any dtype, one row per source element, inner dimensions contiguous, any row
        stride; out: a tensor of the same shape and dtype to fill instead of a new one (only its rows' own bytes are written)"""
        return self._apply(t, kind, nat.ORDER_TO_DECODED, out)

    def to_source(self, t, kind: str = "vertex", out=None):
        """rows in decoded order -> rows in source order: result[i] = t[kind[i]], zero bytes where element i was never coded"""
        return self._apply(t, kind, nat.ORDER_TO_SOURCE, out)


class Bvh(_NamedBuffers):
    """A bounding-volume hierarchy over the triangles of a render build (include/harry_amd.h: hry_bvh_build) and the closest-hit
    ray cast over it (hry_bvh_cast).  The buffers lie in HBM; every bit of them depends on the render build alone, every bit of a
    cast on them and the rays alone.  After a cast: hits (rays that hit), box_tests (box intervals the walk evaluated) and device_ms
    (the kernel) of that cast.  nearest / nearest_numpy: the closest point of the triangles to every query point
    (hry_bvh_nearest), every bit of it on the hierarchy and the points alone."""

    BUFFERS = ("leaf_tri", "leaf_code", "leaf_box", "leaf_positions", "node_children", "node_box", "scene_box")
    SUMMARY = ("triangles", "leaves", "dead", "distinct_codes", "depth")
    _PREFIX, _TYPED = "bvh", True

    def __init__(self, codec: "Codec", handle):
        self.codec, self.h = codec, handle
        self.hits = self.box_tests = self.answered = self.bound_tests = 0
        self.device_ms = self.max_d2 = 0.0

    def count(self) -> int:
        """L: the leaves, the triangles with finite positions"""
        return int(nat.load().hry_bvh_count(self.h))

    def stat(self) -> dict:
        return _read_stat(nat.load(), "bvh", self.h, self.SUMMARY)

    def numpy(self, name: str) -> np.ndarray:
        """one of the buffers as a host array, as buffers_numpy gives it"""
        return _read_buffers(nat.load(), "bvh", self.h, (name,), self.codec._fill_numpy)[name]

    def tensor(self, name: str):
        """one of the buffers as a torch tensor on the codec's device, as buffers gives it"""
        return _read_buffers(nat.load(), "bvh", self.h, (name,), self.codec._torch_fill())[name]

    def buffers_numpy(self) -> dict:
        """the seven buffers as host arrays: leaf_tri, leaf_code u32 [L], leaf_box f32 [L, 6], leaf_positions f32 [L, 9],
        node_children u32 [L - 1, 2] (nat.BVH_LEAF set: a leaf), node_box f32 [L - 1, 6], scene_box f32 [1, 6]"""
        return _read_buffers(nat.load(), "bvh", self.h, self.BUFFERS, self.codec._fill_numpy)

    def buffers(self) -> dict:
        """the same as torch tensors on the codec's device, copied device to device: float32 and int32 (a leaf's child word reads
        negative)"""
        return _read_buffers(nat.load(), "bvh", self.h, self.BUFFERS, self.codec._torch_fill())

    def _cast(self, n, o_ptr, o_stride, d_ptr, d_stride, tmin, tmax, flags, tri_ptr, t_ptr, uv_ptr):
        stat, ms = (C.c_uint64 * 2)(), C.c_double()
        nat.check(nat.load().hry_bvh_cast(self.codec.h, self.h, n, o_ptr, o_stride, d_ptr, d_stride, float(tmin), float(tmax), flags, tri_ptr, t_ptr, uv_ptr,
                                          stat, C.byref(ms)))
        self.hits, self.box_tests, self.device_ms = int(stat[0]), int(stat[1]), ms.value

    @staticmethod
    def _rays(origins, dirs, rows_of):
        """(n, origin stride, direction stride) in bytes for [n, 3] or [3] arrays whose xyz lie together; one origin or direction for
        all rays has the stride 0"""
        (no, so), (nd, sd) = rows_of(origins), rows_of(dirs)
        counts = {c for c in (no, nd) if c not in (None, 1)}
        if len(counts) > 1:
            raise ValueError("origins and dirs: [n, 3] each, or [3] / [1, 3] for one value for all rays")
        return (counts.pop() if counts else 1), (0 if no in (None, 1) else so), (0 if nd in (None, 1) else sd)

    def cast(self, origins, dirs, tmin: float = 0.0, tmax: float = float("inf")) -> dict:
        """the first triangle every ray meets within [tmin, tmax] (hry_bvh_cast).  origins, dirs: float32 torch tensors [n, 3] on the
        codec's device, of any row stride (a view into a wider buffer, an expanded [1, 3]); [3]: one for all rays.  Returns tensors
        there: "tri" int32 [n] (-1: the ray meets nothing), "t" float32 [n] (+inf), "uv" float32 [n, 2] (the barycentric
        coordinates of the second and third corner)"""
        import torch   # only here: the rest of the package does not need torch
        dev = torch.device("cuda", self.codec.device)

        def prepared(t):
            if t.dtype != torch.float32 or t.device != dev or t.dim() not in (1, 2) or t.shape[-1] != 3:
                raise ValueError("rays: float32 tensors [n, 3] or [3] on the codec's device")
            return t if t.stride(-1) == 1 and (t.dim() == 1 or t.stride(0) >= 0) else t.contiguous()

        origins, dirs = prepared(origins), prepared(dirs)
        n, so, sd = self._rays(origins, dirs, lambda t: (None, 0) if t.dim() == 1 else (t.shape[0], t.stride(0) * 4))
        torch.cuda.current_stream(dev).synchronize()   # (the rays may still be in the making on torch's stream)
        tri, t, uv = torch.empty((n,), dtype=torch.int32, device=dev), torch.empty((n,), dtype=torch.float32, device=dev), torch.empty((n, 2), dtype=torch.float32, device=dev)
        self._cast(n, origins.data_ptr(), so, dirs.data_ptr(), sd, tmin, tmax, 0, tri.data_ptr(), t.data_ptr(), uv.data_ptr())
        return {"tri": tri, "t": t, "uv": uv}

    def cast_numpy(self, origins, dirs, tmin: float = 0.0, tmax: float = float("inf")) -> dict:
        """the same from and to host arrays (HRY_CAST_HOST: the library stages them); "tri" is uint32 with NO_ELEMENT for no hit"""
        def prepared(a):
            a = np.asarray(a, np.float32)
            if a.ndim not in (1, 2) or a.shape[-1] != 3:
                raise ValueError("rays: float32 arrays [n, 3] or [3]")
            return a if a.strides[-1] == 4 and (a.ndim == 1 or (a.strides[0] >= 0 and a.strides[0] % 4 == 0)) else np.ascontiguousarray(a)

        origins, dirs = prepared(origins), prepared(dirs)
        n, so, sd = self._rays(origins, dirs, lambda a: (None, 0) if a.ndim == 1 else (a.shape[0], a.strides[0]))
        tri, t, uv = np.empty(n, np.uint32), np.empty(n, np.float32), np.empty((n, 2), np.float32)
        self._cast(n, origins.ctypes.data, so, dirs.ctypes.data, sd, tmin, tmax, nat.CAST_HOST, tri.ctypes.data, t.ctypes.data, uv.ctypes.data)
        return {"tri": tri, "t": t, "uv": uv}

    def _nearest(self, n, q_ptr, q_stride, max_dist, flags, tri_ptr, d2_ptr, uv_ptr, point_ptr):
        stat, ms = (C.c_uint64 * 3)(), C.c_double()
        nat.check(nat.load().hry_bvh_nearest(self.codec.h, self.h, n, q_ptr, q_stride, float(max_dist), flags, tri_ptr, d2_ptr, uv_ptr, point_ptr, stat,
                                             C.byref(ms)))
        self.answered, self.bound_tests, self.device_ms = int(stat[0]), int(stat[1]), ms.value
        self.max_d2 = float(np.uint64(stat[2]).view(np.float64))

    def nearest(self, points, max_dist: float = float("inf")) -> dict:
        """the closest point of the triangles to every query point within max_dist (hry_bvh_nearest).  points: a float32 torch
        tensor [n, 3] on the codec's device, of any row stride (a view into a wider buffer, an expanded [1, 3]); [3]: one point.
        Returns tensors there: "tri" int32 [n] (-1: nothing within max_dist), "d2" float64 [n] (the squared distance; +inf),
        "uv" float32 [n, 2] (the barycentric coordinates of the second and third corner), "point" float32 [n, 3].  Afterwards:
        answered, bound_tests, max_d2 (the largest d2 among the answered points, 0.0 without one) and device_ms"""
        import torch   # only here: the rest of the package does not need torch
        dev = torch.device("cuda", self.codec.device)
        if points.dtype != torch.float32 or points.device != dev or points.dim() not in (1, 2) or points.shape[-1] != 3:
            raise ValueError("points: a float32 tensor [n, 3] or [3] on the codec's device")
        if not (points.stride(-1) == 1 and (points.dim() == 1 or points.stride(0) >= 0)):
            points = points.contiguous()
        n, stride = (1, 0) if points.dim() == 1 else (points.shape[0], points.stride(0) * 4)
        torch.cuda.current_stream(dev).synchronize()   # (the points may still be in the making on torch's stream)
        tri, d2 = torch.empty((n,), dtype=torch.int32, device=dev), torch.empty((n,), dtype=torch.float64, device=dev)
        uv, point = torch.empty((n, 2), dtype=torch.float32, device=dev), torch.empty((n, 3), dtype=torch.float32, device=dev)
        self._nearest(n, points.data_ptr(), stride, max_dist, 0, tri.data_ptr(), d2.data_ptr(), uv.data_ptr(), point.data_ptr())
        return {"tri": tri, "d2": d2, "uv": uv, "point": point}

    def nearest_numpy(self, points, max_dist: float = float("inf")) -> dict:
        """the same from and to host arrays (HRY_NEAREST_HOST: the library stages them); "tri" is uint32 with NO_ELEMENT for an
        unanswered point"""
        points = np.asarray(points, np.float32)
        if points.ndim not in (1, 2) or points.shape[-1] != 3:
            raise ValueError("points: a float32 array [n, 3] or [3]")
        if not (points.strides[-1] == 4 and (points.ndim == 1 or (points.strides[0] >= 0 and points.strides[0] % 4 == 0))):
            points = np.ascontiguousarray(points)
        n, stride = (1, 0) if points.ndim == 1 else (points.shape[0], points.strides[0])
        tri, d2, uv, point = np.empty(n, np.uint32), np.empty(n, np.float64), np.empty((n, 2), np.float32), np.empty((n, 3), np.float32)
        self._nearest(n, points.ctypes.data, stride, max_dist, nat.NEAREST_HOST, tri.ctypes.data, d2.ctypes.data, uv.ctypes.data, point.ctypes.data)
        return {"tri": tri, "d2": d2, "uv": uv, "point": point}

    def intersections(self) -> "Intersections":
        """the pairs of triangles that pass through each other (hry_intersections_build): an owning object of its own, which needs
        neither this hierarchy nor the mesh afterwards"""
        h = C.c_void_p()
        nat.check(nat.load().hry_intersections_build(self.codec.h, self.h, 0, C.byref(h)))   # (one build over the hierarchy alone: no chain)
        return Intersections(self.codec, h)


class Intersections(_NamedBuffers):
    """The pairs of triangles of a hierarchy of which an edge of one meets the other (include/harry_amd.h:
    hry_intersections_build): "pairs" [P, 2] (t < s, ascending), "pair_shared" [P] (the corners they share by position: 0 or 1) and
    "tri_pairs" [T] (the pairs every triangle is in).  The buffers lie in HBM; every bit of them depends on the hierarchy alone.
    candidates: the pairs of leaves whose boxes overlap; tested: those of them that reach the segment tests; pairs: P;
    triangles_hit: the triangles in a pair; box_tests: what the walk evaluated (the one figure that depends on the walk);
    device_ms: the kernels"""

    BUFFERS = ("pairs", "pair_shared", "tri_pairs")
    SUMMARY = ("triangles", "candidates", "tested", "pairs", "triangles_hit", "box_tests")
    _PREFIX, _TYPED = "intersections", True

    def __init__(self, codec: "Codec", handle):
        self.codec, self.h = codec, handle
        st = self.stat()
        self.triangles, self.candidates, self.tested, self.pairs, self.triangles_hit, self.box_tests = (st[k] for k in self.SUMMARY)
        self.device_ms = st["device_ms"]

    def count(self) -> int:
        """P: the pairs"""
        return int(nat.load().hry_intersections_count(self.h))

    def stat(self) -> dict:
        return _read_stat(nat.load(), "intersections", self.h, self.SUMMARY)

    def buffers_numpy(self) -> dict:
        """the three buffers as host arrays: pairs u32 [P, 2], pair_shared u32 [P], tri_pairs u32 [T]"""
        return _read_buffers(nat.load(), "intersections", self.h, self.BUFFERS, self.codec._fill_numpy)

    def buffers(self) -> dict:
        """the same as int32 torch tensors on the codec's device, copied device to device"""
        return _read_buffers(nat.load(), "intersections", self.h, self.BUFFERS, self.codec._torch_fill())


class Distortion(_NamedBuffers):
    """The error of one mesh against another (include/harry_amd.h: hry_distortion_build): per component the largest error and where
    it is, the sum of squared errors, the range of the source's values and the counts; the Euclidean displacement of the positions;
    with rows=True one error value per row ("error<l>") in HBM.  Valid until close(), whatever the codec does later."""

    _PREFIX, _NP, _TORCH = "distortion", np.float32, "float32"

    def __init__(self, codec: "Codec", handle):
        self.codec, self.h = codec, handle

    def component(self, l: int, c: int) -> dict:
        """hry_comp_error of component c of list l, plus rms = sqrt(sum_sq / compared) (0 when nothing was compared)"""
        e = nat.CompError()
        nat.check(nat.load().hry_distortion_component(self.h, l, c, C.byref(e)))
        out = {k: getattr(e, k) for k, _ in e._fields_ if k != "reserved"}
        out["rms"] = math.sqrt(e.sum_sq / e.compared) if e.compared else 0.0
        return out

    def position(self) -> dict:
        """hry_pos_error, plus rms, diagonal (of the box of the source's compared positions) and psnr = 20 log10(diagonal / rms),
        inf when rms is 0; list -1: the meshes have no positions"""
        p = nat.PosError()
        nat.check(nat.load().hry_distortion_position(self.h, C.byref(p)))
        out = {k: getattr(p, k) for k, _ in p._fields_}
        out["rms"] = math.sqrt(p.sum_sq_dist / p.compared) if p.compared else 0.0
        out["diagonal"], out["psnr"] = 0.0, math.inf
        if p.list >= 0:
            first = nat.load().hry_distortion_position_component(self.h)
            comps = [self.component(p.list, first + k) for k in range(3)]
            ext = [max(c["a_max"] - c["a_min"], 0.0) if c["compared"] else 0.0 for c in comps]
            out["diagonal"] = math.sqrt(sum(x * x for x in ext))
            if out["rms"] > 0:
                out["psnr"] = 20.0 * math.log10(out["diagonal"] / out["rms"]) if out["diagonal"] > 0 else -math.inf
        return out

    def normals(self) -> dict:
        """hry_normal_error of a build with normals=True (Codec.distortion_ex): the chord between each face's unit normal before and after (max_chord,
        sum_sq_chord, argmax) and the five face classes, plus max_angle_deg and rms_angle_deg -- the rms is defined as
        chord_angle(sqrt(sum_sq_chord / compared)), the angle of the rms chord.  list -1: no normals; "reason" says why"""
        e = nat.NormalError()
        nat.check(nat.load().hry_distortion_normals(self.h, C.byref(e)))
        out = _normal_record(e)
        if e.list < 0:
            out["reason"] = nat.load().hry_last_error().decode(errors="replace")
        return out

    def rows(self, name: str) -> int:
        """rows of a per-row buffer; 0: there is no such buffer"""
        return super().rows(name)

    def data_ptr(self, name: str) -> int:
        """device address of a per-row buffer (f32 [rows]); 0 when absent"""
        return super().data_ptr(name)

    def numpy(self, name: str) -> np.ndarray:
        """a per-row buffer as a host array (float32)"""
        return super().numpy(name)

    def tensor(self, name: str):
        """a per-row buffer as a torch float32 tensor on the codec's device, copied device to device"""
        return super().tensor(name)

    def stat(self) -> dict:
        """device_ms (the two kernels, by events), uploaded_bytes (records that were not resident)"""
        d, up = C.c_double(), C.c_uint64()
        nat.check(nat.load().hry_distortion_stat(self.h, C.byref(d), C.byref(up)))
        return {"device_ms": d.value, "uploaded_bytes": up.value}


class QuantSweep:
    """The error at every quantisation width (include/harry_amd.h: hry_quant_sweep_build): per swept component and width the record
    Distortion.component gives after a requant of a clone to that width, and per width the positions' displacement.  A host table:
    valid until close(), whatever becomes of the codec."""

    METRICS = {"max_abs": nat.TOL_MAX_ABS, "max_rel": nat.TOL_MAX_REL, "rms": nat.TOL_RMS, "pos_dist": nat.TOL_POS_DIST,
               "normal_chord": nat.TOL_NORMAL_CHORD}

    def __init__(self, handle):
        self.h = handle

    def close(self):
        if getattr(self, "h", None):
            nat.load().hry_quant_sweep_free(self.h)
            self.h = None

    __del__ = close

    def bits(self, l: int, c: int) -> int:
        """the widest width component c of list l was swept at; 0: it was not swept (reason(l, c) says why)"""
        n = nat.load().hry_quant_sweep_bits(self.h, l, c)
        if n < 0:
            nat.check(n)
        return n

    def reason(self, l: int, c: int) -> str:
        """why component c of list l was not swept; '' when it was"""
        return "" if self.bits(l, c) else nat.load().hry_last_error().decode(errors="replace")

    def component(self, l: int, c: int, bits: int) -> dict:
        """hry_comp_error of component c of list l at `bits`, plus rms: the keys of Distortion.component"""
        e = nat.CompError()
        nat.check(nat.load().hry_quant_sweep_component(self.h, l, c, bits, C.byref(e)))
        out = {k: getattr(e, k) for k, _ in e._fields_ if k != "reserved"}
        out["rms"] = math.sqrt(e.sum_sq / e.compared) if e.compared else 0.0
        return out

    def table(self, l: int, c: int) -> list:
        """component(l, c, bits) for bits = 1 .. bits(l, c): entry bits - 1"""
        return [self.component(l, c, q) for q in range(1, self.bits(l, c) + 1)]

    def position(self, bits: int) -> dict:
        """hry_pos_error with the three position components at `bits`, plus rms; list -1: no swept positions"""
        p = nat.PosError()
        nat.check(nat.load().hry_quant_sweep_position(self.h, bits, C.byref(p)))
        out = {k: getattr(p, k) for k, _ in p._fields_}
        out["rms"] = math.sqrt(p.sum_sq_dist / p.compared) if p.compared else 0.0
        return out

    def normals(self, bits: int) -> dict:
        """hry_normal_error with the three position components at `bits` (a sweep built with normals=True; otherwise HryError, "not
        swept"), plus max_angle_deg and rms_angle_deg as Distortion.normals defines them; list -1: not swept, "reason" says why"""
        e = nat.NormalError()
        nat.check(nat.load().hry_quant_sweep_normals(self.h, bits, C.byref(e)))
        out = _normal_record(e)
        if e.list < 0:
            out["reason"] = nat.load().hry_last_error().decode(errors="replace")
        return out

    def choose(self, tolerances) -> list:
        """tolerances: iterable of (list, component or -1, metric, value); metric: "max_abs", "max_rel", "rms", "pos_dist",
        "normal_chord" (value: angle_chord of the largest angle between a face's normals, list the position list, component -1) or a
        nat.TOL_* number.  Returns [(list, component, bits), ...] for Codec.requant: per named component the smallest width that
        meets its tolerances, 0 (lossless) when none does"""
        ts = []
        for l, c, m, v in tolerances:
            if isinstance(m, str) and m not in self.METRICS:
                raise HryError(nat.E_ARG, f"unknown tolerance metric {m!r}")
            ts.append(nat.Tolerance(int(l), int(c), self.METRICS[m] if isinstance(m, str) else int(m), 0, float(v)))
        arr = (nat.Tolerance * max(len(ts), 1))(*ts)
        n = C.c_size_t()
        cap = 32 * 16 + 16
        out = (nat.Quant * cap)()
        nat.check(nat.load().hry_quant_choose(self.h, arr, len(ts), out, cap, C.byref(n)))
        return [(out[i].list, out[i].comp, out[i].bits) for i in range(n.value)]

    def stat(self) -> dict:
        """device_ms (the two kernels, by events), uploaded_bytes (records that were not resident)"""
        d, up = C.c_double(), C.c_uint64()
        nat.check(nat.load().hry_quant_sweep_stat(self.h, C.byref(d), C.byref(up)))
        return {"device_ms": d.value, "uploaded_bytes": up.value}


def rate_hist_bytes(hist) -> float:
    """hry_rate_hist_bytes: the zeroth-order entropy of a 256-bin histogram, in bytes"""
    h = np.ascontiguousarray(hist, np.uint32)
    if h.shape != (256,):
        raise HryError(nat.E_ARG, "a histogram has 256 bins")
    out = C.c_double()
    nat.check(nat.load().hry_rate_hist_bytes(h.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(out)))
    return out.value


def rate_pick(bytes_by_bits, budget: float, n_bits: int | None = None) -> int:
    """hry_rate_pick: the largest width in 1 .. n_bits whose entry (index bits - 1) is at most `budget`; 0: none"""
    t = np.ascontiguousarray(bytes_by_bits, np.float64).reshape(-1)
    n = len(t) if n_bits is None else n_bits
    buf = t if len(t) else np.zeros(1)
    bits = nat.load().hry_rate_pick(buf.ctypes.data_as(C.POINTER(C.c_double)), n, float(budget))
    if bits < 0:
        nat.check(bits)
    return bits


class RateSweep:
    """The coded size at every quantisation width (include/harry_amd.h: hry_rate_sweep_build): per component of list 1 and width the
    histogram of every byte plane of its residual codes -- np.bincount of the encoder's "vplanes" stage after a requant of a clone
    to that width; width 0: the component as it stands.  A host table: valid until close(), whatever becomes of the codec."""

    def __init__(self, handle):
        self.h = handle

    def close(self):
        if getattr(self, "h", None):
            nat.load().hry_rate_sweep_free(self.h)
            self.h = None

    __del__ = close

    @property
    def coded(self) -> int:
        """coded vertices: what every histogram sums to"""
        return int(nat.load().hry_rate_sweep_coded(self.h))

    def bits(self, l: int, c: int) -> int:
        """the widest width component c of list l was swept at; 0: it was not swept (reason(l, c) says why)"""
        n = nat.load().hry_rate_sweep_bits(self.h, l, c)
        if n < 0:
            nat.check(n)
        return n

    def reason(self, l: int, c: int) -> str:
        return "" if self.bits(l, c) else nat.load().hry_last_error().decode(errors="replace")

    def planes(self, l: int, c: int, bits: int) -> int:
        n = nat.load().hry_rate_sweep_planes(self.h, l, c, bits)
        if n < 0:
            nat.check(n)
        return n

    def hist(self, l: int, c: int, bits: int) -> np.ndarray:
        """[planes, 256] uint32: the histograms of the component's byte planes at `bits` (0: as it stands)"""
        out = np.zeros((self.planes(l, c, bits), 256), np.uint32)
        for p in range(out.shape[0]):
            nat.check(nat.load().hry_rate_sweep_hist(self.h, l, c, bits, p, out[p].ctypes.data_as(C.POINTER(C.c_uint32))))
        return out

    def bytes(self, l: int, c: int, bits: int) -> float:
        """the entropy of the component's planes at `bits`, in bytes: an estimate of its share of the payload"""
        out = C.c_double()
        nat.check(nat.load().hry_rate_sweep_bytes(self.h, l, c, bits, C.byref(out)))
        return out.value

    def choose(self, l: int, c: int, budget: float):
        """(bits, bytes): the largest common width of component c of list l (-1: every swept one) whose estimate fits `budget`; bits 0: none"""
        bits, est = C.c_int(), C.c_double()
        nat.check(nat.load().hry_rate_choose(self.h, l, c, float(budget), C.byref(bits), C.byref(est)))
        return bits.value, est.value

    def stat(self) -> dict:
        """device_ms (the kernel, by events), walk_ms (the host's walk), uploaded_bytes (a mesh that was not resident)"""
        d, w, up = C.c_double(), C.c_double(), C.c_uint64()
        nat.check(nat.load().hry_rate_sweep_stat(self.h, C.byref(d), C.byref(w), C.byref(up)))
        return {"device_ms": d.value, "walk_ms": w.value, "uploaded_bytes": up.value}


class MultiCodec:
    """Several device contexts driven from this one process (include/harry_amd.h: hry_encode_sharded / hry_decode_sharded): the
    reference's single entry with N devices behind it.  devices: one index per context; an index may repeat (contexts that share
    a device run side by side on it)."""

    def __init__(self, devices):
        self.ctx = [Codec(int(d)) for d in devices]
        self.last = {}

    def close(self):
        for c in getattr(self, "ctx", []):
            c.close()
        self.ctx = []

    __del__ = close

    def _handles(self):
        return (C.c_void_p * len(self.ctx))(*[c.h for c in self.ctx])

    def write_hry(self, mesh: Mesh, quants=(), clear: bool = False, n_shards: int = 0, chunk_syms: int = 0, keep_mesh: bool = False, as_buffer: bool = False,
                  return_order: bool = False):
        """plan + extract + bounds of the whole mesh + quantisation + encode of every shard on its context + merge: ONE .hry v0.3.
        keep_mesh: do not store the combined bounds in `mesh`; return_order: refused (E_UNSUPPORTED): a sharded encode builds no numbering maps"""
        qs = list(quants)
        arr = (nat.Quant * max(len(qs), 1))(*[nat.Quant(int(l), int(c), int(b)) for l, c, b in qs])
        o = nat.Opts(PROFILE_CHUNKED, chunk_syms, 0, (FLAG_KEEP_MESH if keep_mesh else 0) | (FLAG_ORDER if return_order else 0), 0, int(n_shards))
        p, n, t = C.c_void_p(), C.c_size_t(), nat.ShardTiming()
        nat.check(nat.load().hry_encode_sharded(self._handles(), len(self.ctx), mesh.h, arr, len(qs), int(clear), C.byref(o), C.byref(p), C.byref(n), C.byref(t)))
        self.last = t.asdict()
        return nat.take(p, n.value, as_buffer)

    def read_hry(self, data: bytes, shard=(0, 0), partial: bool = False) -> Mesh:
        o = nat.Opts(0, 0, 0, FLAG_PARTIAL if partial else 0, int(shard[0]), int(shard[1]))
        h, t = C.c_void_p(), nat.ShardTiming()
        nat.check(nat.load().hry_decode_sharded(self._handles(), len(self.ctx), data, len(data), C.byref(o), C.byref(h), C.byref(t)))
        self.last = t.asdict()
        return Mesh(h)

    def timings(self):
        return [c.timing() for c in self.ctx]


def container_check(data: bytes) -> bool:
    """host-only validation of a sharded container's directory; returns whether its runs cover the whole mesh"""
    c = C.c_int()
    nat.check(nat.load().hry_container_check(data, len(data), C.byref(c)))
    return bool(c.value)


def parse_quant_flags(flags):
    """The reference CLI's -l/-a/-q/-c state machine (main.cc:47-71) -> ([(list, comp, bits)], clear)."""
    cur_l, cur_a, out, clear = None, -1, [], False
    it = iter(flags)
    for f in it:
        if f in ("-l", "--list"):
            cur_l = int(next(it))
        elif f.startswith("-l") and f[2:].lstrip("-").isdigit():
            cur_l = int(f[2:])
        elif f in ("-a", "--attr"):
            cur_a = int(next(it))
        elif f.startswith("-a") and f[2:].lstrip("-").isdigit():
            cur_a = int(f[2:])
        elif f in ("-q", "--quant"):
            out.append((cur_l, cur_a, int(next(it)))); cur_a = -1
        elif f.startswith("-q") and f[2:].lstrip("-").isdigit():
            out.append((cur_l, cur_a, int(f[2:]))); cur_a = -1
        elif f in ("-c", "--clear-quant"):
            clear = True
        else:
            raise ValueError(f"unknown flag {f}")
    for l, _, _ in out:
        if l is None:
            raise ValueError("-q without a preceding -l (the reference reads an uninitialised list index here, main.cc:48)")
    return out, clear
