"""Restatement in numpy of the numbering maps of an encode (include/harry_amd.h: hry_order_take) from the host walk's arrays, and
of the mesh a decode must return: the source permuted by the maps.  tests/test_order_cpu.py pins both to the oracle's own decode
of its own encode; tests/test_gpu_order.py compares the device's maps and the product's decode with them, array for array.

The decoder numbers vertices in the order they are introduced (order_v: the half-edge at which), faces in coding order (order_f:
the half-edge through which a face is entered), and makes that half-edge the face's first: the corners keep their cyclic order."""
from __future__ import annotations

import numpy as np

NO = 0xFFFFFFFF


TYPE_SIZE = (4, 8, 8, 8, 4, 4, 2, 2, 1, 1)   # mixing::Type: float, double, ulong, long, uint, int, ushort, short, uchar, char


def stored(mesh, l: int) -> np.ndarray:
    """The records of list l as the codec stores them: of every component's slot the bytes of its STORAGE type -- a component
    quantised to q bits lives in the low 1 / 2 / 4 / 8 bytes of a slot as wide as its original type, and what a requantisation
    leaves in the slot's other bytes is no part of the value (a decode returns them zero)."""
    data = mesh.list_data(l).reshape(mesh.list_count(l), -1)
    keep = np.zeros(data.shape[1], bool)
    for t, q, off in mesh.list_fmt(l):
        st = t if q == 0 else 8 if q <= 8 else 6 if q <= 16 else 4 if q <= 32 else 2
        keep[off:off + TYPE_SIZE[st]] = True
    return np.where(keep[None, :], data, 0).astype(np.uint8)


def inverse(x: np.ndarray, rows: int) -> np.ndarray:
    """inv[x[i]] = i over the coded elements; rows that nothing maps to hold NO"""
    inv = np.full(rows, NO, np.uint32)
    coded = np.flatnonzero(x != NO)
    inv[x[coded]] = coded
    return inv


def maps_from_walk(mesh, order_v, order_f) -> dict:
    """mesh: an object with nv, nf, ne, face_offsets(), org() (harry_amd.codec.Mesh); order_v / order_f: the walk's arrays"""
    nv, nf, ne = mesh.nv, mesh.nf, mesh.ne
    foff = np.asarray(mesh.face_offsets(), np.int64)
    org = np.asarray(mesh.org(), np.int64)
    order_v, order_f = np.asarray(order_v, np.int64), np.asarray(order_f, np.int64)
    deg = np.diff(foff)
    eface = np.repeat(np.arange(nf, dtype=np.int64), deg)
    vertex = np.full(nv, NO, np.uint32)
    vertex[org[order_v]] = np.arange(len(order_v), dtype=np.uint32)
    face = np.full(nf, NO, np.uint32)
    face[eface[order_f]] = np.arange(len(order_f), dtype=np.uint32)
    # decoded face j is source face eface[order_f[j]]: the decoded offsets are the scan of those degrees
    doff = np.concatenate(([0], np.cumsum(deg[eface[order_f]])))
    corner = np.full(ne, NO, np.uint32)
    c = np.flatnonzero(face[eface] != NO)
    j = face[eface[c]].astype(np.int64)
    corner[c] = doff[j] + (c - order_f[j]) % deg[eface[c]]   # places behind the entering half-edge, round the face
    out = {"vertex": vertex, "face": face, "corner": corner}
    for name, rows in (("vertex", nv), ("face", nf), ("corner", ne)):
        out[name + "_inv"] = inverse(out[name], rows)
    return out


def record_maps_from_walk(mesh, order_v, order_f) -> dict:
    """general bindings: "list<l>" and its inverse for every list.  The decoder numbers a list's records in creation order: the
    order in which the coding order first names them -- vertices in order_v, faces in order_f, a face's corners from the entering
    half-edge on round the face; at one element, slot by slot."""
    foff = np.asarray(mesh.face_offsets(), np.int64)
    org = np.asarray(mesh.org(), np.int64)
    order_v, order_f = np.asarray(order_v, np.int64), np.asarray(order_f, np.int64)
    deg = np.diff(foff)
    eface = np.repeat(np.arange(mesh.nf, dtype=np.int64), deg)
    vreg, freg = mesh.regions_of(1).astype(np.int64), mesh.regions_of(0).astype(np.int64)
    bind = [mesh.bindings(k) for k in range(3)]
    # the corners in coding order: face by face, from order_f[j] on round the face
    fj = eface[order_f]
    start = np.concatenate(([0], np.cumsum(deg[fj])))
    k = np.arange(start[-1]) - np.repeat(start[:-1], deg[fj])
    corners = np.repeat(foff[fj], deg[fj]) + (np.repeat(order_f - foff[fj], deg[fj]) + k) % np.repeat(deg[fj], deg[fj])
    elems = {0: (fj, freg[fj]), 1: (org[order_v], vreg[org[order_v]]), 2: (corners, freg[eface[corners]])}
    out = {}
    for l in range(mesh.nlists):
        tg = mesh.list_target(l)
        rows = mesh.list_count(l)
        x = np.full(rows, NO, np.uint32)
        if tg in elems:
            el, reg = elems[tg]
            nreg = mesh.nregions(1 if tg == 1 else 0)
            slots = max([len(mesh.region_lists(tg, r)) for r in range(nreg)] + [0])
            named = np.full((len(el), slots), -1, np.int64)   # the records an element names in list l, slot by slot
            for r in range(nreg):
                for a, bound in enumerate(mesh.region_lists(tg, r)):
                    if bound == l:
                        sel = reg == r
                        named[sel, a] = bind[tg][el[sel], a]
            seq = named.reshape(-1)
            seq = seq[seq >= 0]
            first = np.unique(seq, return_index=True)
            created = first[0][np.argsort(first[1], kind="stable")]   # records in order of first naming
            x[created] = np.arange(len(created), dtype=np.uint32)
        out[f"list{l}"] = x
        out[f"list{l}_inv"] = inverse(x, rows)
    return out


def permuted_connectivity(mesh, maps, twin=None) -> dict:
    """face_offsets, org and (when the mesh's twins after the encode are given) twin of the decode, from the maps"""
    foff = np.asarray(mesh.face_offsets(), np.int64)
    org = np.asarray(mesh.org(), np.int64)
    deg = np.diff(foff)
    vertex, corner, finv = maps["vertex"], maps["corner"], maps["face_inv"]
    out = {}
    ddeg = np.where(finv != NO, deg[np.minimum(finv, max(len(deg) - 1, 0))], 0) if len(deg) else np.zeros(0, np.int64)
    out["face_offsets"] = np.concatenate(([0], np.cumsum(ddeg))).astype(np.uint32)
    c = np.flatnonzero(corner != NO)
    d_org = np.zeros(mesh.ne, np.uint32)
    d_org[corner[c]] = vertex[org[c]]
    out["org"] = d_org
    if twin is not None:
        d_twin = np.zeros(mesh.ne, np.uint32)
        d_twin[corner[c]] = corner[np.asarray(twin, np.int64)[c]]
        out["twin"] = d_twin
    return out


def permuted(mesh, maps, twin=None) -> dict:
    """What a decode of an encode of `mesh` (PLY layout) returns, from the maps: face_offsets, org, twin (when given: the mesh's
    twins after the encode), vrec / frec (the vertex and face records; rows that no source element maps to are zero)"""
    out = permuted_connectivity(mesh, maps, twin)
    vertex, face = maps["vertex"], maps["face"]
    for key, l, m in (("vrec", 1, vertex), ("frec", 0, face)):
        src = stored(mesh, l)
        dst = np.zeros_like(src)
        e = np.flatnonzero(m != NO)
        dst[m[e]] = src[e]
        out[key] = dst
    return out


def decoded_arrays(dec) -> dict:
    """the same arrays of a decoded mesh (harry_amd.codec.Mesh or the oracle's)"""
    out = {"face_offsets": np.asarray(dec.face_offsets(), np.uint32), "org": np.asarray(dec.org(), np.uint32),
           "vrec": stored(dec, 1), "frec": stored(dec, 0)}
    return out


def check_general_decode(src, dec, maps) -> None:
    """general bindings: `dec` (a decode of an encode of `src`) is `src` moved through the maps -- record bytes through "list<l>",
    the binding tables of all three kinds through the element maps and the record maps, regions through "vertex" / "face".  Asserts."""
    assert (dec.nv, dec.nf, dec.ne, dec.nlists) == (src.nv, src.nf, src.ne, src.nlists)
    for l in range(src.nlists):
        x = maps[f"list{l}"]
        a, b = stored(src, l), stored(dec, l)
        assert a.shape == b.shape and src.list_fmt(l) == dec.list_fmt(l), l
        r = np.flatnonzero(x != NO)
        assert np.array_equal(b[x[r]], a[r]), f"records of list {l}"
    deg = np.diff(np.asarray(src.face_offsets(), np.int64))
    eface = np.repeat(np.arange(src.nf, dtype=np.int64), deg)
    sfreg, dfreg, svreg, dvreg = src.regions_of(0), dec.regions_of(0), src.regions_of(1), dec.regions_of(1)
    face, vertex, corner = maps["face"], maps["vertex"], maps["corner"]
    assert np.array_equal(dfreg[face], sfreg), "face regions"
    v = np.flatnonzero(vertex != NO)
    assert np.array_equal(dvreg[vertex[v]], svreg[v]), "vertex regions"
    for kind, emap, reg in ((0, face, sfreg.astype(np.int64)), (1, vertex, svreg.astype(np.int64)), (2, corner, sfreg.astype(np.int64)[eface])):
        sb, db = src.bindings(kind), dec.bindings(kind)
        assert sb.shape[0] == db.shape[0], kind   # (slots that no region binds need not survive: the OBJ reader always makes two corner slots)
        e = np.flatnonzero(emap != NO)
        checked = 0
        for r in range(src.nregions(1 if kind == 1 else 0)):
            sel = e[reg[e] == r]
            for a, l in enumerate(src.region_lists(kind, r)):
                want = maps[f"list{l}"][sb[sel, a]]
                assert not (want == NO).any(), (kind, r, a)   # (a record that an element names is coded)
                assert np.array_equal(db[emap[sel], a], want), f"bindings of kind {kind}, region {r}, slot {a}"
                checked += len(sel)
        assert checked or not sb.size or not e.size
