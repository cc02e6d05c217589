"""numpy restatement of the weld of hry_mesh_from_device (include/harry_amd.h: HRY_INGEST_WELD), shared by the ingest tests."""
from __future__ import annotations

import numpy as np


def packed_records(columns) -> np.ndarray:
    """uint8 [n, stride]: the components of every row, as stored, back to back in the order given (the list's layout order)"""
    cols = [np.ascontiguousarray(c) for c in columns]
    n = len(cols[0])
    return np.concatenate([c.view(np.uint8).reshape(n, c.dtype.itemsize) for c in cols], axis=1) if cols else np.zeros((n, 0), np.uint8)


def weld(records: np.ndarray):
    """rows with equal bytes share one vertex, numbered in order of first occurrence: (output vertex of every row u32 [n], first row
    of every output vertex u32 [nout])"""
    records = np.ascontiguousarray(records, np.uint8)
    n = len(records)
    if n == 0:
        return np.zeros(0, np.uint32), np.zeros(0, np.uint32)
    keys = records.view(np.dtype((np.void, records.shape[1]))).reshape(n)
    _, first, inv = np.unique(keys, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")
    rank = np.empty(len(order), np.int64)
    rank[order] = np.arange(len(order))
    return rank[inv.reshape(-1)].astype(np.uint32), first[order].astype(np.uint32)
