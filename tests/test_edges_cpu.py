"""hry_edges_build without a GPU: the entry points exist and refuse null arguments, the ABI is still 6, and the numpy restatement
the GPU tests compare against (tests/edges_ref.py) gives known answers on meshes small enough to do by hand."""
import ctypes as C

import numpy as np

from harry_amd import _native as nat
from tests import edges_ref as er

NONE = er.NO_ELEMENT


def test_entry_points_and_abi():
    L = nat.load()
    assert L.hry_abi_version() == 6
    for name in ("build", "count", "get", "copy", "summary", "stat", "free"):
        assert hasattr(L, "hry_edges_" + name), name
    out = C.c_void_p(1)
    assert L.hry_edges_build(None, None, None, 0, C.byref(out)) == nat.E_ARG and not out.value and L.hry_last_error()
    assert L.hry_edges_build(None, None, None, 0, None) == nat.E_ARG
    rows = C.c_uint64(7)
    assert L.hry_edges_get(None, b"edges", None, C.byref(rows), None, None) == nat.E_ARG
    assert L.hry_edges_copy(None, None, b"edges", None, 0) == nat.E_ARG
    assert L.hry_edges_summary(None, (C.c_uint64 * 4)()) == nat.E_ARG
    assert L.hry_edges_stat(None, None, None) == nat.E_ARG
    assert L.hry_edges_count(None) == 0
    L.hry_edges_free(None)
    assert nat.EDGES_GEOMETRY == 1


def build(pos, tris, vs=None):
    pos = np.asarray(pos, np.float32)
    return er.build(np.asarray(tris, np.uint32), np.arange(len(pos)) if vs is None else vs, pos)


def test_single_triangle():
    r = build([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 1, 2]])
    assert r["summary"] == (3, 3, 0, 0)
    assert np.array_equal(r["edges"], [[0, 1], [1, 2], [0, 2]]) and np.array_equal(r["tri_edges"], [[0, 1, 2]])
    assert np.array_equal(r["edge_offsets"], [0, 1, 2, 3]) and np.array_equal(r["edge_sides"], [0, 1, 2])
    assert (r["tri_neighbours"] == NONE).all() and (r["edge_cos"] == 2.0).all()
    assert np.array_equal(r["edge_length"], np.array([1, np.sqrt(2.0), 1], np.float32))
    assert np.array_equal(r["edge_cot"], np.array([0.5, 0, 0.5], np.float32))   # the angle opposite each edge: 45, 90 (at vertex 0), 45 degrees


def test_two_triangles_wound_consistently_and_against():
    pos = [[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]]
    r = build(pos, [[0, 1, 2], [2, 1, 3]])
    assert r["summary"] == (5, 4, 1, 0)
    shared = int(r["tri_edges"][0, 1])
    assert shared == int(r["tri_edges"][1, 0]) and np.array_equal(r["edge_sides"][r["edge_offsets"][shared]:r["edge_offsets"][shared + 1]], [1, 3])
    assert r["edge_cos"][shared] == 1.0 and (np.delete(r["edge_cos"], shared) == 2.0).all()
    assert r["tri_neighbours"][0, 1] == 1 and r["tri_neighbours"][1, 0] == 0 and (r["tri_neighbours"] == NONE).sum() == 4
    # the second triangle turned over: the normals are opposed (-1), both sides run 1 -> 2, and the negation gives +1
    r = build(pos, [[0, 1, 2], [1, 2, 3]])
    shared = int(r["tri_edges"][0, 1])
    assert shared == int(r["tri_edges"][1, 0]) and r["edge_cos"][shared] == 1.0
    # folded flat onto each other, wound consistently: -1
    r = build([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 1, 0]], [[0, 1, 2], [1, 0, 3]])
    assert r["edge_cos"][int(r["tri_edges"][0, 0])] == -1.0


def cube():
    pos = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    tris = [t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))]
    return pos, np.array(tris, np.uint32)


def test_unit_cube():
    pos, tris = cube()
    r = build(pos, tris)
    E, one, two, more = r["summary"]
    assert (E, one, two, more) == (18, 0, 18, 0) and len(pos) - E + len(tris) == 2
    assert set(r["edge_cos"].tolist()) == {0.0, 1.0} and (r["edge_cos"] == 1.0).sum() == 6   # the six face diagonals
    assert (r["tri_neighbours"] != NONE).all()
    assert np.array_equal(np.sort(r["edge_length"]), np.sort(np.array([1.0] * 12 + [np.sqrt(2.0)] * 6, np.float32)))
    assert (r["edge_cot"][r["edge_cos"] == 1.0] == 0.0).all()   # a diagonal faces two right angles


def test_equilateral_triangle():
    r = build([[1, 0, 0], [0, 1, 0], [0, 0, 1]], [[0, 1, 2]])   # exact coordinates: u . v = 1 and |u x v| = sqrt(3) at every corner
    assert np.array_equal(r["edge_cot"], np.full(3, 0.5 / np.sqrt(3.0)).astype(np.float32))
    assert np.array_equal(r["edge_length"], np.full(3, np.sqrt(2.0)).astype(np.float32))


def test_repeated_index_triangle():
    r = build([[0, 0, 0], [1, 0, 0]], [[0, 1, 1]])
    assert r["summary"] == (2, 1, 1, 0)
    assert np.array_equal(r["edges"], [[0, 1], [1, 1]]) and np.array_equal(r["tri_edges"], [[0, 1, 0]])   # a self-edge, like any other
    assert np.array_equal(r["edge_sides"], [0, 2, 1]) and np.array_equal(r["tri_neighbours"], [[0, NONE, 0]])
    assert (r["edge_cos"] == 2.0).all() and np.array_equal(r["edge_cot"].view(np.uint32), [0, 0])   # exactly +0
    assert np.array_equal(r["edge_length"], [1, 0])


def test_seam_is_one_edge():
    """two output vertices of one decoded vertex on either side of a seam: the key is the decoded pair"""
    pos = [[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [1, 0, 0], [0, 1, 0]]
    vs = np.array([0, 1, 2, 3, 1, 2])
    r = er.build(np.array([[0, 1, 2], [5, 4, 3]], np.uint32), vs, np.asarray(pos, np.float32))
    assert r["summary"] == (5, 4, 1, 0)
    shared = int(r["tri_edges"][0, 1])
    assert np.array_equal(r["edges"][shared], [1, 2]) and r["edge_cos"][shared] == 1.0


def test_float_steps():
    a = np.array([1.0, -0.0, np.nan, 2.0], np.float32)
    assert er.float_steps(a, a) == (0, 0.0)
    b = a.copy()
    b[0] = np.nextafter(np.float32(1), np.float32(2))
    assert er.float_steps(a, b) == (1, 1.0)
    b[2] = 0
    assert er.float_steps(a, b)[1] == np.inf
