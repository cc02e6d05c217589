"""hry_shells_build without a GPU: the entry points exist and refuse null arguments, the ABI is still 6, and the numpy restatement
the GPU tests compare against (tests/shells_ref.py) gives known answers on cases done by hand and on the generator's meshes."""
import ctypes as C

import numpy as np

from harry_amd import _native as nat
from harry_amd import meshgen as mg
from tests import edges_ref as er
from tests import shells_ref as sr

COL = {k: i for i, k in enumerate(sr.COLUMNS)}


def test_entry_points_and_abi():
    L = nat.load()
    assert L.hry_abi_version() == 6
    for name in ("build", "count", "get", "copy", "summary", "stat", "free"):
        assert hasattr(L, "hry_shells_" + name), name
    out = C.c_void_p(1)
    assert L.hry_shells_build(None, None, None, None, 0, C.byref(out)) == nat.E_ARG and not out.value and L.hry_last_error()
    assert L.hry_shells_build(None, None, None, None, 0, None) == nat.E_ARG
    rows = C.c_uint64(7)
    assert L.hry_shells_get(None, b"tri_shell", None, C.byref(rows), None, None) == nat.E_ARG
    assert L.hry_shells_copy(None, None, b"tri_shell", None, 0) == nat.E_ARG
    assert L.hry_shells_summary(None, (C.c_uint64 * 6)()) == nat.E_ARG
    assert L.hry_shells_stat(None, None, None) == nat.E_ARG
    assert L.hry_shells_count(None) == 0
    L.hry_shells_free(None)
    assert nat.SHELLS_GEOMETRY == 1


def build(pos, tris, vs=None):
    pos = np.asarray(pos, np.float32)
    tris = np.asarray(tris, np.uint32).reshape(-1, 3)
    vs = np.arange(len(pos)) if vs is None else vs
    return sr.build(tris, vs, np.arange(len(tris)), len(tris), er.build(tris, vs), pos)


def cube(at=(0, 0, 0)):
    pos = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float32) + np.asarray(at, np.float32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    return pos, np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.int64)


def test_single_triangle():
    r = build([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 1, 2]])
    assert r["shell_counts"].tolist() == [[1, 1, 3, 3, 3, 0, 0, 1]] and r["summary"] == (1, 0, 0, 0, 1, 1)
    assert r["tri_shell"].tolist() == [0] and r["shell_first"].tolist() == [0] and r["edge_shell"].tolist() == [0, 0, 0]
    assert r["shell_measures"][0].tolist() == [0.5, 0, 0, 0, 0, 1, 1, 0]
    assert sr.euler(r["shell_counts"][0]) == 1 and sr.genus(r["shell_counts"][0]) == 0


def test_no_triangles():
    r = build(np.zeros((0, 3)), np.zeros((0, 3)))
    assert r["summary"] == (0, 0, 0, 0, 0, 0) and all(r[k].shape[0] == 0 for k in sr.FIXED + sr.GEOMETRY)


def test_unit_cube_and_inside_out():
    pos, tris = cube()
    r = build(pos, tris)
    row = r["shell_counts"][0]
    assert r["summary"] == (1, 1, 0, 0, 0, 12) and row.tolist() == [12, 12, 8, 18, 0, 0, 0, 0]
    assert sr.euler(row) == 2 and sr.genus(row) == 0
    assert r["shell_measures"][0].tolist() == [6, 1, 0, 0, 0, 1, 1, 1]          # area 6 and volume 1, exactly
    far = build(pos + np.float32(4096), tris)                                       # O is a vertex of the shell: nothing cancels
    assert far["shell_measures"][0, :2].tolist() == [6, 1]
    r = build(pos, tris[:, ::-1])
    assert r["shell_measures"][0, :2].tolist() == [6, -1] and r["shell_counts"][0, COL["misoriented"]] == 0


def test_two_cubes_touching_at_a_vertex():
    pa, ta = cube()
    pb, tb = cube((1, 1, 1))
    remap = np.concatenate([[7], np.arange(8, 15)])                                 # B's corner (1, 1, 1) is A's
    pos = np.concatenate([pa, pb[1:]])
    r = build(pos, np.concatenate([ta, remap[tb]]))
    assert len(pos) == 15 and r["summary"] == (2, 2, 0, 0, 0, 12)
    assert r["shell_counts"][:, COL["vertices"]].tolist() == [8, 8]                 # the shared vertex counts in both
    assert r["tri_shell"].tolist() == [0] * 12 + [1] * 12 and r["shell_first"].tolist() == [0, 12]
    assert [sr.euler(row) for row in r["shell_counts"]] == [2, 2]
    assert r["shell_measures"][1].tolist() == [6, 1, 1, 1, 1, 2, 2, 2]


def test_two_cubes_sharing_an_edge():
    pa, ta = cube()
    pb, tb = cube((1, 1, 0))
    remap = np.concatenate([[6, 7], np.arange(8, 14)])                              # B's edge (1, 1, z) is A's
    r = build(np.concatenate([pa, pb[2:]]), np.concatenate([ta, remap[tb]]))
    row = r["shell_counts"][0]
    assert r["summary"] == (1, 0, 1, 0, 0, 24) and row[COL["nonmanifold"]] == 1 and row[COL["vertices"]] == 14 and row[COL["edges"]] == 35
    assert sr.genus(row) is None


def moebius(n=12):
    """a band of n quads whose ends meet with a half turn: vertices a_i = 2 i, b_i = 2 i + 1"""
    a = lambda i: 2 * i if i < n else 1
    b = lambda i: 2 * i + 1 if i < n else 0
    tris = [t for i in range(n) for t in ((a(i), a(i + 1), b(i + 1)), (a(i), b(i + 1), b(i)))]
    u = 2 * np.pi * np.arange(n) / n
    mid = np.stack([np.cos(u), np.sin(u), 0 * u], axis=1)
    off = 0.3 * np.stack([np.cos(u / 2) * np.cos(u), np.cos(u / 2) * np.sin(u), np.sin(u / 2)], axis=1)
    pos = np.empty((2 * n, 3))
    pos[0::2], pos[1::2] = mid + off, mid - off
    return pos, tris


def test_moebius_strip():
    r = build(*moebius())
    row = r["shell_counts"][0]
    assert r["summary"][0] == 1 and row[COL["misoriented"]] >= 1 and row[COL["loops"]] == 1 and row[COL["boundary"]] == 24
    assert sr.euler(row) == 0 and sr.genus(row) is None and r["summary"][3] == 1


def test_seam_does_not_cut():
    pos = [[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [1, 0, 0], [0, 1, 0]]
    r = build(pos, [[0, 1, 2], [5, 4, 3]], vs=np.array([0, 1, 2, 3, 1, 2]))
    assert r["summary"] == (1, 0, 0, 0, 1, 2) and r["shell_counts"][0].tolist() == [2, 2, 4, 5, 4, 0, 0, 1]


def test_loops_of_touching_shells_stay_apart():
    """two triangles that share one vertex: two shells, a loop each (a hook per vertex alone would join them)"""
    r = build([[0, 0, 0], [1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0]], [[0, 1, 2], [0, 3, 4]])
    assert r["summary"] == (2, 0, 0, 0, 2, 1) and r["shell_counts"][:, COL["loops"]].tolist() == [1, 1]
    # ... and a bow tie inside ONE shell is one loop by the rule: its two cycles share a decoded vertex
    r = build([[0, 0, 0], [1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0], [1, 1, 0]], [[0, 1, 2], [0, 3, 4], [1, 5, 2]])
    assert r["summary"][0] == 2


def test_box_and_degenerate_terms():
    pos = [[0, 0, 0], [2, 0, 0], [0, 2, 0], [4, 0, 0], [np.nan, -0.0, 1], [np.inf, 0.0, -3]]
    # good, a repeated index, collinear corners, a NaN corner, an infinite corner: one shell through the edge 0 - 1
    r = build(pos, [[0, 1, 2], [0, 1, 1], [0, 1, 3], [1, 0, 4], [0, 1, 5]])
    m = r["shell_measures"][0]
    assert r["summary"][0] == 1 and m[0] == 2.0 and m[1] == 0.0 and m[:2].view(np.uint32)[1] == 0    # the other terms are exactly +0
    assert m[2:].tolist() == [0, 0, -3, 4, 2, 1] and np.signbit(m[3])                                 # -0 is below +0; NaN and inf are skipped
    r = build([[np.nan] * 3] * 3, [[0, 1, 2]])
    assert r["shell_measures"][0].tolist() == [0, 0, np.inf, np.inf, np.inf, -np.inf, -np.inf, -np.inf]


def test_chunked_association_is_what_the_header_says():
    """300 + 300 interleaved triangles: the sums are per chunk of 256 first, then over the chunks -- not one running sum"""
    rng = np.random.default_rng(11)
    n = 300
    pos = rng.standard_normal((2 * (n + 2), 3)).astype(np.float32)
    a = np.array([[i, i + 1, i + 2] if i % 2 == 0 else [i + 1, i, i + 2] for i in range(n)])
    tris = np.stack([a, a + n + 2], axis=1).reshape(-1, 3)
    r = build(pos, tris)
    assert r["summary"][0] == 2 and (r["tri_shell"] == np.arange(2 * n) % 2).all()
    P = pos.astype(np.float64)
    t = np.flatnonzero(r["tri_shell"] == 1)
    I = tris[t]
    term = er._norm(er._cross(P[I[:, 1]] - P[I[:, 0]], P[I[:, 2]] - P[I[:, 0]]))
    total = np.float64(0)
    for c in range(0, 2 * n, 256):
        part = np.float64(0)
        for x in term[(t >= c) & (t < c + 256)]:
            part = part + x
        total = total + part
    assert r["shell_measures"][1, 0] == np.float32(0.5 * total)


# ---- the generator's meshes: what the GPU test's expectations stand on
def rows(m):
    r = sr.of_mesh(m, geometry=False)
    return r, r["shell_counts"]


def test_torus_triangles_and_mixed():
    r, c = rows(mg.torus(24, 16))
    assert r["summary"][0] == 1 and sr.euler(c[0]) == 0 and c[0, COL["loops"]] == 0 and sr.genus(c[0]) == 1
    m = mg.torus(24, 16, polys="mixed")
    r2, c2 = rows(m)
    assert c2[0, COL["triangles"]] == 768 and c2[0, COL["faces"]] == 584 == len(m.degrees)
    assert np.array_equal(np.delete(c2, COL["faces"], axis=1), np.delete(c, COL["faces"], axis=1)) and r2["summary"] == r["summary"]


def test_grid_icosphere_nonmanifold_soup():
    r, c = rows(mg.grid(9, 8, quads=True))
    assert r["summary"][0] == 1 and c[0, COL["boundary"]] == 30 and c[0, COL["loops"]] == 1 and sr.euler(c[0]) == 1
    r, c = rows(mg.icosphere(2))
    assert r["summary"][:2] == (1, 1) and sr.euler(c[0]) == 2 and sr.genus(c[0]) == 0
    r, c = rows(mg.with_nonmanifold(mg.torus(12, 10)))
    assert r["summary"][0] == 2 and c[0, [COL["triangles"], COL["nonmanifold"], COL["boundary"], COL["loops"]]].tolist() == [242, 2, 4, 2]
    assert c[1, COL["triangles"]] == 1
    r, c = rows(mg.soup())
    assert r["summary"][0] == 39 and r["summary"][5] == 25 and (c[:, COL["misoriented"]] > 0).sum() > 1


def test_components_holes_discs_ribbons():
    r, c = rows(mg.multi_component(3, 8, 6))
    assert r["summary"][0] == 3 and [sr.euler(x) for x in c] == [0, 0, 0]
    r, c = rows(mg.with_holes(mg.torus(24, 16), 5))
    assert r["summary"][0] == 1 and c[0, COL["boundary"]] == 15 and c[0, COL["loops"]] == 4 and sr.euler(c[0]) == -5
    r, c = rows(mg.hub_discs([5, 7, 40]))
    assert r["summary"][0] == 3 and c[:, COL["loops"]].tolist() == [1, 1, 1] and [sr.euler(x) for x in c] == [1, 1, 1]
    r, c = rows(mg.ribbon(30))
    assert c[0, COL["loops"]] == 2 and sr.euler(c[0]) == 0
    r, c = rows(mg.ribbon(30, closed=False))
    assert c[0, COL["loops"]] == 1 and sr.euler(c[0]) == 1
