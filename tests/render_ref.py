"""numpy restatement of the render-ready buffers (include/harry_amd.h: hry_render_build), shared by the render tests."""
from __future__ import annotations

import numpy as np

NONE = 0xFFFFFFFF


def unwelded(mesh) -> bool:
    """general bindings where some face region binds a corner list"""
    return bool(mesh.general) and any(len(mesh.region_lists(2, r)) for r in range(mesh.nregions(0)))


def corner_keys(mesh) -> np.ndarray:
    """(ne, 1 + corner lists) u32: org, then per corner-target list in list order the record the corner names, or NONE"""
    foff = mesh.face_offsets().astype(np.int64)
    eface = np.repeat(np.arange(mesh.nf), np.diff(foff))
    clists = [l for l in range(mesh.nlists) if mesh.list_target(l) == 2]
    keys = np.full((mesh.ne, 1 + len(clists)), NONE, np.uint32)
    keys[:, 0] = mesh.org()
    freg, cb = mesh.regions_of(0), mesh.bindings(2)
    for r in range(mesh.nregions(0)):
        sel = freg[eface] == r
        for a, l in enumerate(mesh.region_lists(2, r)):
            if l in clists:
                keys[sel, 1 + clists.index(l)] = cb[sel, a]
    return keys


def first_occurrence(keys: np.ndarray):
    """rows with equal keys share one id; ids in order of first occurrence.  Returns (id of every row, first row of every id)."""
    keys = np.ascontiguousarray(keys)
    _, first, inv = np.unique(keys, axis=0, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")
    rank = np.empty(len(order), np.int64)
    rank[order] = np.arange(len(order))
    return rank[inv.reshape(-1)].astype(np.uint32), first[order].astype(np.uint32)


def vertex_map(mesh):
    """(corner -> output vertex, vertex_source, corner_source or None)"""
    if unwelded(mesh):
        cmap, csrc = first_occurrence(corner_keys(mesh))
        return cmap, mesh.org()[csrc], csrc
    return mesh.org(), np.arange(mesh.nv, dtype=np.uint32), None


def fan(foff: np.ndarray, vmap: np.ndarray):
    """(indices [T, 3], tri_face [T]): triangle k of face f is (c0, c(k+1), c(k+2))"""
    foff = foff.astype(np.int64)
    nf = len(foff) - 1
    deg = np.diff(foff)
    tri_face = np.repeat(np.arange(nf, dtype=np.int64), deg - 2)
    t = np.arange(len(tri_face), dtype=np.int64)
    k = t - (foff[:-1] - 2 * np.arange(nf))[tri_face]
    c0 = foff[tri_face]
    idx = np.stack([vmap[c0], vmap[c0 + k + 1], vmap[c0 + k + 2]], axis=1).astype(np.uint32)
    return idx, tri_face.astype(np.uint32)
