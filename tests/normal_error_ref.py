"""Restatement in numpy of the faces' normal deviation (include/harry_amd.h: hry_normal_error, hry_distortion_build with
HRY_DISTORTION_NORMALS, hry_quant_sweep_build_ex with HRY_SWEEP_NORMALS).  Input: two double arrays [rows, 3] -- the positions after
requant(clear=True), as tests/distortion_ref.values gives them, from code that is not under test -- the faces, the map between the
rows and, with general bindings, the row of every vertex.  Every operation is an individually rounded double operation in the
contract's order (the _cross / _length idiom of tests/normals_ref.py), so max_chord, argmax, the counters and the per-face chords
are exact; sum_sq_chord is math.fsum of the individually rounded c2: the exact sum of the terms, rounded once.

The meshes of tests/test_normal_sweep_cpu.py and tests/test_gpu_normal_sweep.py are built here too, once per process."""
from __future__ import annotations

import functools
import math

import numpy as np

from harry_amd import meshgen as mg
from tests import distortion_ref as dref
from tests import quant_sweep_ref as qref
from tests.normals_ref import _cross, _length, _usable

NO = dref.NO
FIELDS = ("max_chord", "sum_sq_chord", "compared", "skipped", "nonfinite", "degenerate", "collapsed", "argmax")
EXACT = tuple(k for k in FIELDS if k != "sum_sq_chord")


def fan_normals(pc: np.ndarray, deg: np.ndarray, lo: np.ndarray) -> np.ndarray:
    """pc: a position per corner [ne, 3].  N_f: the fan triangles' cross products relative to corner 0, in order"""
    N = np.zeros((len(deg), 3))
    if len(deg):
        p0 = pc[lo]
        for k in range(1, int(deg.max()) - 1):
            sel = np.nonzero(deg > k + 1)[0]
            t = _cross(pc[lo[sel] + k] - p0[sel], pc[lo[sel] + k + 1] - p0[sel])
            N[sel] = t if k == 1 else N[sel] + t
    return N


def compare(x: np.ndarray, y: np.ndarray, degrees, indices, map_=None, rows=None) -> dict:
    """x [rows_a, 3], y [rows_b, 3]: the positions; degrees u8 [nf], indices: the flattened corners (vertex ids); map_: uint32
    [rows_a] (NO: none), None: the identity; rows: uint32 [nv], the row of every vertex in the position list (NO: none), None: row v.
    Returns the fields of hry_normal_error without `list`, and "faces": float32 [nf], the chord of a compared face and 0 elsewhere"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    deg = np.asarray(degrees).astype(np.int64)
    org = np.asarray(indices).astype(np.int64)
    nf = len(deg)
    off = np.concatenate([[0], np.cumsum(deg)])
    lo = off[:-1]
    face = np.repeat(np.arange(nf), deg)
    ra = org.copy() if rows is None else np.asarray(rows, np.uint32).astype(np.int64)[org]
    none = ra == NO
    if map_ is None:
        rb = ra.copy()
    else:
        rb = np.asarray(map_, np.uint32).astype(np.int64)[np.where(none, 0, ra)]
        none |= rb == NO
    assert (rb[~none] < len(y)).all(), "a map entry at or above b's count"
    ra, rb = np.where(none, 0, ra), np.where(none, 0, rb)
    skipped = np.zeros(nf, bool)
    np.logical_or.at(skipped, face, none)
    with np.errstate(all="ignore"):
        xa, yb = x[ra], y[rb]
        bad = ~(np.isfinite(xa).all(axis=1) & np.isfinite(yb).all(axis=1))
        nonfinite = np.zeros(nf, bool)
        np.logical_or.at(nonfinite, face, bad)
        nonfinite &= ~skipped
        Nx, Ny = fan_normals(xa, deg, lo), fan_normals(yb, deg, lo)
        lx, ly = _length(Nx), _length(Ny)
        rest = ~skipped & ~nonfinite
        degenerate = rest & ~_usable(lx)
        collapsed = rest & ~degenerate & ~_usable(ly)
        ok = rest & ~degenerate & ~collapsed
        d = Ny[ok] / ly[ok][:, None] - Nx[ok] / lx[ok][:, None]
        c2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        chord = np.sqrt(c2)
    rec = {"max_chord": 0.0, "sum_sq_chord": math.fsum(c2.tolist()), "compared": int(ok.sum()), "skipped": int(skipped.sum()),
           "nonfinite": int(nonfinite.sum()), "degenerate": int(degenerate.sum()), "collapsed": int(collapsed.sum()), "argmax": NO}
    if rec["compared"]:
        rec["max_chord"] = float(chord.max())
        rec["argmax"] = int(np.flatnonzero(ok)[np.flatnonzero(chord == chord.max())[0]])   # the lowest face that attains it
    faces = np.zeros(nf, np.float32)
    faces[ok] = chord.astype(np.float32)
    rec["faces"] = faces
    assert rec["compared"] + rec["skipped"] + rec["nonfinite"] + rec["degenerate"] + rec["collapsed"] == nf
    return rec


def table(values_at, x: np.ndarray, pos: int, qmax: int, degrees, indices, rows=None) -> list:
    """values_at(comps, bits) -> [rows, ncomp] as in tests/quant_sweep_ref.py; x: the source's values [rows, ncomp].  The records
    with components pos .. pos + 2 all at 1 .. qmax bits: entry bits - 1"""
    cols = [pos, pos + 1, pos + 2]
    return [compare(x[:, cols], values_at(cols, q)[:, cols], degrees, indices, rows=rows) for q in range(1, qmax + 1)]


def meets(rec: dict, value: float) -> bool:
    return rec["max_chord"] <= value and rec["collapsed"] == 0


def pick(tab: list, value: float) -> int:
    """the smallest bits whose record meets the chord and has no collapsed face; 0: none does"""
    for bits, rec in enumerate(tab, 1):
        if meets(rec, value):
            return bits
    return 0


def chord_of_degrees(deg: float) -> float:
    return 2.0 * math.sin(math.radians(deg) / 2.0)


# ---- the meshes (meshgen meshes: structured vertices, degrees, indices).  The smallest at which the kernels can go wrong
@functools.lru_cache(maxsize=None)
def mesh(name: str) -> mg.Mesh:
    if name == "tri":      # 1 600 vertices, 3 200 triangles: four blocks of 1 024 faces with a ragged last one; no face offsets are read
        return mg.torus(40, 40)
    if name == "mixed":    # the general-degree gather: degrees 3, 4, 5 and one 64-gon, a flat regular disc on 64 new vertices
        t = mg.torus(24, 24, polys="mixed")
        n = 64
        a = 2.0 * np.pi * np.arange(n) / n
        disc = np.zeros(n, t.verts.dtype)
        disc["x"], disc["y"], disc["z"] = (0.3 * np.cos(a)).astype(np.float32), (0.3 * np.sin(a)).astype(np.float32), np.float32(0.6)
        return mg.Mesh(np.concatenate([t.verts, disc]), np.concatenate([t.degrees, np.array([n], np.uint8)]),
                       np.concatenate([t.indices, t.nv + np.arange(n, dtype=np.uint32)]))
    if name in ("ushort", "int", "double"):   # tri's positions in another type: the type switch; qmax 16 / 30 / 30
        t = mesh("tri")
        p = np.stack([t.verts[k].astype(np.float64) for k in "xyz"], axis=1)
        if name == "double":
            cols = {k: p[:, i] * (1.0 + 2.0 ** -40) for i, k in enumerate("xyz")}   # (not representable as floats)
        else:
            dt, top = (np.uint16, 65535.0) if name == "ushort" else (np.int32, 1.0e6)
            lo, ext = p.min(), p.max() - p.min()
            s = np.round((p - lo) / ext * top)
            if name == "int":
                s -= 5.0e5
            cols = {k: s[:, i].astype(dt) for i, k in enumerate("xyz")}
        return mg.Mesh(mg._vtx_struct(cols), t.degrees, t.indices)
    if name in ("bad", "bad_inf"):   # one x NaN, two vertices moved onto a third: nonfinite and degenerate faces.  bad_inf: one x +inf
        t = mesh("tri")              # too -- the POS group's shared extent is infinite, and every face is nonfinite at every width
        v = t.verts.copy()
        v["x"][100] = np.nan
        if name == "bad_inf":
            v["x"][900] = np.inf
        v[421] = v[420]
        v[461] = v[420]
        return mg.Mesh(v, t.degrees, t.indices)
    raise KeyError(name)


def vertex_rows(m, pl: int) -> np.ndarray:
    """general bindings (a codec or oracle mesh): the record of list pl that every vertex names, NO where its region does not bind it"""
    reg, attr = m.regions_of(1), m.bindings(1)
    rows = np.full(len(reg), NO, np.uint32)
    for r in np.unique(reg):
        lists = m.region_lists(1, int(r))
        if pl in lists:
            rows[reg == r] = attr[reg == r, lists.index(pl)]
    return rows


@functools.lru_cache(maxsize=None)
def obj_scene(colors=None) -> bytes:
    """a small textured scene with general bindings: mixed degrees, corner lists, two materials.  colors "some": every third vertex
    lies in a second vertex region with a list of its own (x y z r g b) -- no one list holds every vertex's position"""
    from harry_amd import objgen as og
    return og.scene(mg.torus(12, 14, polys="mixed"), normals="smooth", tex="atlas", charts=3, materials=2, colors=colors).obj


def positions(m) -> np.ndarray:
    """the positions of a mesh object (oracle or codec, quantisation cleared) as doubles [rows, 3]: the first three components of list 1"""
    return dref.values(m, 1)[:, :3]
