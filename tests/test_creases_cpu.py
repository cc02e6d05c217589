"""What of the creases build needs no GPU: the entry points of hry_creases_build (include/harry_amd.h), and the restatement of its
contract (tests/creases_ref.py) against closed forms.  The meshes here are (positions [nv, 3] float32, degrees, corners), as in
tests/seam_meshes.py; tests/test_gpu_creases.py builds the same ones on the device."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from harry_amd import _native as nat
from harry_amd import meshgen as mg
from tests import creases_ref as cr
from tests import normals_ref as nr
from tests import seam_meshes as sm
from tests import shells_ref as sr
from tests import util

HEADER = os.path.join(util.ROOT, "include", "harry_amd.h")
NAMES = ("build", "count", "get", "copy", "summary", "stat", "free")
CLASSES = ("SMOOTH", "SHARP", "BOUNDARY", "NONMANIFOLD", "MISORIENTED", "DEGENERATE")
WEIGHTS = ("area", "angle")


def test_header_declares_and_library_exports():
    text = open(HEADER).read()
    L = nat.load()
    for name in NAMES:
        assert re.search(r"\bhry_creases_%s\(" % name, text), name
        assert hasattr(L, "hry_creases_" + name), name
    assert "typedef struct hry_creases hry_creases;" in text
    assert re.search(r"uint64_t hry_creases_count\(const hry_creases \*", text)
    assert re.search(r"#define HRY_CREASES_ANGLE_WEIGHTED\s+1u\b", text) and nat.CREASES_ANGLE_WEIGHTED == 1
    for value, name in enumerate(CLASSES):
        assert re.search(r"#define HRY_CREASE_%s\s+%du\b" % (name, value), text), name
        assert getattr(nat, "CREASE_" + name) == value == getattr(cr, name)
    assert re.search(r"#define HRY_ABI_VERSION\s+6\b", text) and L.hry_abi_version() == 6


def test_null_arguments_without_a_device():
    L = nat.load()
    out = C.c_void_p(1)
    assert L.hry_creases_build(None, None, None, None, 0.5, 0, C.byref(out)) == nat.E_ARG and not out.value
    assert L.hry_creases_build(None, None, None, None, 0.5, 0, None) == nat.E_ARG
    assert L.hry_creases_count(None) == 0
    s = (C.c_uint64 * 6)()
    assert L.hry_creases_summary(None, s) == nat.E_ARG and L.hry_creases_stat(None, None, None) == nat.E_ARG
    rows = C.c_uint64()
    assert L.hry_creases_get(None, b"normals", None, C.byref(rows), None, None) == nat.E_ARG
    L.hry_creases_free(None)


# ---- the meshes
CUBE_POS = [[x, y, z] for z in (0, 1) for y in (0, 1) for x in (0, 1)]   # vertex x + 2 y + 4 z
CUBE_QUADS = [[0, 2, 3, 1], [4, 5, 7, 6], [0, 1, 5, 4], [2, 6, 7, 3], [0, 4, 6, 2], [1, 3, 7, 5]]   # counter-clockwise seen from outside
AXES = np.float32([[0, 0, -1], [0, 0, 1], [0, -1, 0], [0, 1, 0], [-1, 0, 0], [1, 0, 0]])            # the quads' outward normals


def cube_quads():
    return np.float32(CUBE_POS), np.full(6, 4, np.uint8), np.array(CUBE_QUADS, np.uint32).reshape(-1)


def cube_triangles():
    tris = [t for q in CUBE_QUADS for t in ([q[0], q[1], q[2]], [q[0], q[2], q[3]])]
    return np.float32(CUBE_POS), np.full(12, 3, np.uint8), np.array(tris, np.uint32).reshape(-1)


def prism(n):
    """an n-gonal prism of height 1: the caps are fans of n triangles about a centre, the sides are n quads.  Vertices: the bottom
    ring 0 .. n-1, the top ring n .. 2n-1, the bottom centre 2n, the top centre 2n + 1; the faces: bottom cap, top cap, sides"""
    a = 2 * np.pi * np.arange(n) / n
    ring = np.stack([np.cos(a), np.sin(a)], axis=1)
    pos = np.concatenate([np.c_[ring, np.zeros(n)], np.c_[ring, np.ones(n)], [[0, 0, 0], [0, 0, 1]]]).astype(np.float32)
    i = np.arange(n)
    j = (i + 1) % n
    bottom = np.stack([np.full(n, 2 * n), j, i], axis=1)
    top = np.stack([np.full(n, 2 * n + 1), n + i, n + j], axis=1)
    sides = np.stack([i, j, n + j, n + i], axis=1)
    deg = np.concatenate([np.full(2 * n, 3), np.full(n, 4)]).astype(np.uint8)
    return pos, deg, np.concatenate([bottom.reshape(-1), top.reshape(-1), sides.reshape(-1)]).astype(np.uint32)


def prism_limits(n):
    """(a limit at which the sides are smooth and the rims sharp, one at which the sides are sharp too and the caps still smooth)"""
    return math.cos(math.radians(80)), (math.cos(2 * math.pi / n) + 1) / 2


def seam_fan():
    """four triangles about decoded vertex 0, nearly flat; the fan is cut open along the edge 0 - 1 as a uv seam cuts it: the last two
    triangles name output vertices 5 and 6, duplicates of 0 and 1 -> (positions [7, 3], triangles, vertex_source)"""
    pos = np.float32([[0, 0, 0.2], [1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0], [0, 0, 0.2], [1, 0, 0]])
    return pos, np.array([[0, 1, 2], [0, 2, 3], [5, 3, 4], [5, 4, 6]], np.uint32), np.array([0, 1, 2, 3, 4, 0, 1])


def turned(mesh, t):
    """a triangle mesh with triangle t wound the other way"""
    pos, deg, idx = mesh
    tris = np.array(idx).reshape(-1, 3)
    tris[t] = tris[t][[0, 2, 1]]
    return pos, deg, tris.reshape(-1)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- the restatement against closed forms
@pytest.mark.parametrize("weights", WEIGHTS)
def test_unit_cube_of_quads(weights):
    r = cr.of_arrays(*cube_quads(), 0.0, weights)   # edge_cos is exactly 0: smooth at equality
    assert r["summary"] == (8, 8, 18, 0, 0, 0) and r["guard"].all()
    assert np.array_equal(r["render_vertex"][r["indices"]], sr.fan(*cube_quads()[1:])[0])   # the same triangles, renumbered
    for limit in (np.nextafter(0.0, 1.0), math.cos(math.radians(90))):
        r = cr.of_arrays(*cube_quads(), limit, weights)
        assert r["summary"] == (24, 24, 6, 12, 8, 0) and r["guard"].all()
        assert sorted(r["edge_class"].tolist()) == [cr.SMOOTH] * 6 + [cr.SHARP] * 12
        # every corner of quad f is a split vertex of its own with the quad's normal, exactly
        for f in range(6):
            w = np.unique(r["indices"][2 * f:2 * f + 2])
            assert len(w) == 4 and np.array_equal(r["normals"][w], np.tile(AXES[f], (4, 1))), f
        assert np.array_equal(r["vertex_source"], r["render_vertex"])


def test_cube_of_triangle_faces():
    r = cr.of_arrays(*cube_triangles(), 1.0)   # the diagonals' cosine is exactly 1: smooth at equality, the cube's edges sharp
    assert r["summary"] == (24, 24, 6, 12, 8, 0)
    assert cr.of_arrays(*cube_triangles(), 2.0)["summary"] == (36, 36, 0, 18, 8, 0)   # flat shading
    assert cr.of_arrays(*cube_triangles(), -1.0)["summary"] == (8, 8, 18, 0, 0, 0)


@pytest.mark.parametrize("n", [6, 32, 33, 40])
def test_prism(n):
    smooth_sides, sharp_sides = prism_limits(n)
    for weights in WEIGHTS:
        a = cr.of_arrays(*prism(n), smooth_sides, weights)
        assert a["summary"][:2] == (4 * n + 2, 4 * n + 2) and a["summary"][2:] == (4 * n, 2 * n, 2 * n, 0) and a["guard"].all()
        b = cr.of_arrays(*prism(n), sharp_sides, weights)
        assert b["summary"][:2] == (6 * n + 2, 6 * n + 2) and b["summary"][2:] == (3 * n, 3 * n, 2 * n, 0) and b["guard"].all()
        for r in (a, b):
            # the caps: triangles 0 .. n-1 below, n .. 2n-1 above; the centres' groups have n slots
            assert np.array_equal(r["normals"][r["indices"][:n].reshape(-1)], np.tile(np.float32([0, 0, -1]), (3 * n, 1)))
            assert np.array_equal(r["normals"][r["indices"][n:2 * n].reshape(-1)], np.tile(np.float32([0, 0, 1]), (3 * n, 1)))
            assert sorted(r["group_slots"].tolist())[-2:] == [n, n]


@pytest.mark.parametrize("name", ["torus", "icosphere"])
def test_smooth_closed_surfaces_are_the_render_normals(name):
    m = mg.torus(24, 16) if name == "torus" else mg.icosphere(2)
    assert (m.degrees == 3).all()
    for weights in WEIGHTS:
        r = cr.of_mesh(m, -1.0, weights)
        want = nr.of_mesh(m, weights)[1]
        assert r["summary"][0] == m.nv and r["summary"][3:] == (0, 0, 0) and r["guard"].all()
        # the same triangles over the same vertices, renumbered by first use: W = U and render_vertex is a permutation
        assert np.array_equal(r["render_vertex"][r["indices"]], m.indices.reshape(-1, 3)) and np.array_equal(np.sort(r["render_vertex"]), np.arange(m.nv))
        assert np.array_equal(bits(r["normals"]), bits(want[r["render_vertex"]])), weights


def test_turned_face():
    mesh = sm.gen_arrays(mg.torus(24, 16))
    t = 100
    base, r = cr.of_arrays(*mesh, -1.0), cr.of_arrays(*turned(mesh, t), -1.0)
    nv = len(mesh[0])
    assert r["summary"] == (nv + 3, nv + 3, base["summary"][2] - 3, 0, 3, 3)
    assert (r["edge_class"] == cr.MISORIENTED).sum() == 3
    corners = np.array(mesh[2]).reshape(-1, 3)[t]
    # the turned triangle stands alone at its three vertices, with its own (turned) normal ...
    own = r["normals"][r["indices"][t]]
    assert len(np.unique(r["indices"][t])) == 3 and np.array_equal(bits(own), bits(np.tile(own[0], (3, 1))))
    assert (np.bincount(r["indices"].reshape(-1))[r["indices"][t]] == 1).all()
    # ... and no other vertex's row changes a bit
    away = ~np.isin(base["vertex_source"][base["indices"]], corners)
    assert away.sum() == 3 * len(base["indices"]) - 18
    assert np.array_equal(bits(r["normals"][r["indices"][away]]), bits(base["normals"][base["indices"][away]]))
    assert np.array_equal(r["vertex_source"][r["indices"][away]], base["vertex_source"][base["indices"][away]])


def test_uv_seam_splits_the_vertex_but_not_the_normal():
    pos, tris, vs = seam_fan()
    for weights in WEIGHTS:
        r = cr.build(tris, vs, np.arange(4), pos, -1.0, weights)
        assert r["summary"] == (7, 5, 4, 0, 0, 4) and r["guard"].all()
        a, b = r["indices"][0, 0], r["indices"][2, 0]   # decoded vertex 0 on either side of the seam
        assert a != b and (r["render_vertex"][a], r["render_vertex"][b]) == (0, 5) and r["vertex_source"][a] == r["vertex_source"][b] == 0
        assert r["slot_group"][0, 0] == r["slot_group"][2, 0] and np.array_equal(bits(r["normals"][a]), bits(r["normals"][b]))
        assert r["normals"][a].any()
        # ... and a limit that makes everything sharp still leaves the seam's two sides their own normals
        flat = cr.build(tris, vs, np.arange(4), pos, 2.0, weights)
        assert flat["summary"][:4] == (12, 12, 0, 4)
