"""numpy restatement of hry_mesh_from_device_corners (include/harry_amd.h), shared by its tests: the per-list weld (built on
tests/ingest_ref.py), the face regions numbered by first occurrence, and the binding tables the constructor must produce."""
from __future__ import annotations

import numpy as np

from tests import ingest_ref as ir


def weld_rows(rows: np.ndarray):
    """float32 [n, k] -> (output record of every row u32 [n], welded rows [nout, k]): rows equal byte for byte merge, output records
    numbered in order of first occurrence"""
    rows = np.ascontiguousarray(rows, np.float32)
    remap, first = ir.weld(ir.packed_records([rows[:, j] for j in range(rows.shape[1])]))
    return remap, rows[first]


def regions_by_first_occurrence(materials) -> np.ndarray:
    """u16 [nf]: the distinct values numbered in the order they first appear over the faces"""
    materials = np.asarray(materials).astype(np.int64)
    if materials.size == 0:
        return np.zeros(0, np.uint16)
    _, first, inv = np.unique(materials, return_index=True, return_inverse=True)
    rank = np.empty(len(first), np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(len(first))
    return rank[inv.reshape(-1)].astype(np.uint16)


def corner_attr(ne: int, uv_idx=None, normal_idx=None, uv_remap=None, normal_remap=None) -> np.ndarray:
    """u32 [ne, 2]: slot 0 is the texture list's row and the next slot the normal list's, compacted (normals alone sit in slot 0); an
    unused slot holds 0; indices go through the list's weld map when one is given"""
    out = np.zeros((ne, 2), np.uint32)
    slot = 0
    for idx, remap in ((uv_idx, uv_remap), (normal_idx, normal_remap)):
        if idx is None:
            continue
        idx = np.asarray(idx).reshape(-1).astype(np.int64)
        out[:, slot] = idx if remap is None else np.asarray(remap)[idx]
        slot += 1
    return out


def vtx_attr(nv: int) -> np.ndarray:
    """u32 [nv, 1]: vertex v names record v of list 0"""
    return np.arange(nv, dtype=np.uint32).reshape(nv, 1)


def expected(pos, pos_idx, uv=None, uv_idx=None, normals=None, normal_idx=None, materials=None, weld=False) -> dict:
    """what the constructor returns for these arrays: lists (float32 rows), remaps (None without weld), org, corner_attr, vtx_attr,
    face_reg (None without materials: all zero)"""
    lists, remaps = [], []
    for rows in (pos, uv, normals):
        if rows is None:
            lists.append(None); remaps.append(None)
        elif weld:
            r, w = weld_rows(rows)
            lists.append(w); remaps.append(r)
        else:
            lists.append(np.ascontiguousarray(rows, np.float32)); remaps.append(None)
    pos_idx = np.asarray(pos_idx).reshape(-1).astype(np.int64)
    ne = len(pos_idx)
    org = (pos_idx if remaps[0] is None else remaps[0][pos_idx]).astype(np.uint32)
    ui = None if uv is None else (pos_idx if uv_idx is None else uv_idx)
    ni = None if normals is None else (pos_idx if normal_idx is None else normal_idx)
    return {"lists": lists, "remaps": remaps, "org": org, "corner_attr": corner_attr(ne, ui, ni, remaps[1], remaps[2]),
            "vtx_attr": vtx_attr(len(lists[0])), "face_reg": None if materials is None else regions_by_first_occurrence(materials)}
