"""Restatement in numpy of hry_distortion_build (include/harry_amd.h): the per-component error of one mesh against another through
a numbering map.  Input: two double arrays [rows, ncomp] -- the components' values after requant(clear=True), which code that is
not under test produces (the oracle's requant in tests/test_distortion_cpu.py, Codec.requant, pinned to the reference's goldens, in
tests/test_gpu_distortion.py) -- and the map.  Output: the fields of hry_comp_error per component, hry_pos_error, the per-row error.
Sums come from math.fsum of the individually rounded e*e: the exact sum of the terms, rounded once."""
from __future__ import annotations

import math

import numpy as np

NO = 0xFFFFFFFF


def values(mesh, l: int) -> np.ndarray:
    """the components of list l of a mesh whose quantisation has been cleared, as doubles [rows, ncomp]: floats widen exactly,
    64-bit integers round to nearest (numpy's astype)"""
    fmt = mesh.list_fmt(l)
    assert all(q == 0 for _, q, _ in fmt), "values() reads a mesh after requant(clear=True)"
    rows = mesh.list_count(l)
    if not fmt:
        return np.zeros((rows, 0), np.float64)
    return np.stack([np.asarray(mesh.component(l, c)).astype(np.float64) for c in range(len(fmt))], axis=1).reshape(rows, len(fmt))


def compare(x: np.ndarray, y: np.ndarray, map_=None, pos: int | None = None) -> dict:
    """x [rows_a, ncomp], y [rows_b, ncomp]: doubles; map_: uint32 [rows_a] (NO: skipped), None: the identity; pos: the first of the
    three position components, or None.  Returns {"comp": [fields of hry_comp_error per component], "pos": fields of hry_pos_error
    without `list` (None without pos), "rows": float32 [rows_a]}"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    rows, ncomp = x.shape
    map_ = np.arange(rows, dtype=np.uint32) if map_ is None else np.asarray(map_, np.uint32)
    assert map_.shape == (rows,)
    mapped = map_ != NO
    assert (map_[mapped] < len(y)).all(), "a map entry at or above b's count"
    at = np.flatnonzero(mapped)
    skipped = int(rows - len(at))
    xa, yb = x[at], y[map_[at]]
    finite = np.isfinite(xa) & np.isfinite(yb)
    with np.errstate(invalid="ignore", over="ignore"):
        e = yb - xa
        sq = e * e
    comp = []
    row_acc = np.zeros(len(at), np.float64)
    for c in range(ncomp):
        ok = finite[:, c]
        ec, sc, ac = e[ok, c], sq[ok, c], xa[ok, c]
        rec = {"max_abs": 0.0, "sum_sq": math.fsum(sc.tolist()), "a_min": math.inf, "a_max": -math.inf, "compared": int(ok.sum()),
               "skipped": skipped, "nonfinite": int((~ok).sum()), "argmax": NO}
        differ = xa[~ok, c].view(np.uint64) != yb[~ok, c].view(np.uint64)
        rec["changed"] = int((ec != 0).sum()) + int(differ.sum())
        if rec["compared"]:
            mags = np.abs(ec)
            rec["max_abs"] = float(mags.max())
            rec["argmax"] = int(at[ok][np.flatnonzero(mags == mags.max())[0]])   # the lowest row that attains it
            rec["a_min"], rec["a_max"] = float(ac.min()), float(ac.max())
        comp.append(rec)
        row_acc = np.where(ok, row_acc + sq[:, c], row_acc)   # in component order, compared pairs only
    out_rows = np.zeros(rows, np.float32)
    out_rows[at] = np.sqrt(row_acc).astype(np.float32)
    p = None
    if pos is not None:
        ok = finite[:, pos] & finite[:, pos + 1] & finite[:, pos + 2]
        d2 = ((sq[:, pos] + sq[:, pos + 1]) + sq[:, pos + 2])[ok]
        p = {"max_dist": 0.0, "sum_sq_dist": math.fsum(d2.tolist()), "compared": int(ok.sum()), "argmax": NO}
        if p["compared"]:
            dist = np.sqrt(d2)
            p["max_dist"] = float(dist.max())
            p["argmax"] = int(at[ok][np.flatnonzero(dist == dist.max())[0]])
    return {"comp": comp, "pos": p, "rows": out_rows}


def sum_tolerance(rows: int) -> float:
    """relative bound on any summation order of `rows` non-negative, individually rounded terms against their exact sum:
    (rows - 1) * 2^-53 * (1 + o(1)), taken as rows * 2^-52"""
    return rows * 2.0 ** -52
