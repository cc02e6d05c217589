"""What of the curvature build needs no GPU: the entry points of hry_curvature_build (include/harry_amd.h), and the restatement of its
contract (tests/curvature_ref.py) against closed forms.  The meshes here are (positions [nv, 3] float32, degrees, corners), as in
tests/seam_meshes.py; tests/test_gpu_curvature.py builds the same ones on the device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from harry_amd import _native as nat
from harry_amd import meshgen as mg
from tests import curvature_ref as cv
from tests import edges_ref as er
from tests import shells_ref as sr
from tests import util
from tests.test_creases_cpu import cube_quads, cube_triangles

HEADER = os.path.join(util.ROOT, "include", "harry_amd.h")
NAMES = ("build", "count", "get", "copy", "summary", "totals", "stat", "free")
ULP = 2.0 ** -52


def test_header_declares_and_library_exports():
    text = open(HEADER).read()
    L = nat.load()
    for name in NAMES:
        assert re.search(r"\bhry_curvature_%s\(" % name, text), name
        assert hasattr(L, "hry_curvature_" + name), name
    assert "typedef struct hry_curvature hry_curvature;" in text
    assert re.search(r"hry_curvature_build\s+\(no counterpart:", text)
    for name, value in (("ISOLATED", 0), ("INTERIOR", 1), ("BOUNDARY", 2), ("IRREGULAR", 3), ("DEGENERATE", 8)):
        assert re.search(r"#define HRY_VERTEX_%s\s+%du\b" % (name, value), text), name
        assert getattr(nat, "VERTEX_" + name) == value == getattr(cv, name)


def test_null_arguments_without_a_device():
    L = nat.load()
    out = C.c_void_p(1)
    assert L.hry_curvature_build(None, None, None, None, 0, C.byref(out)) == nat.E_ARG and not out.value
    assert L.hry_curvature_build(None, None, None, None, 0, None) == nat.E_ARG
    assert L.hry_curvature_count(None) == 0
    s, t = (C.c_uint64 * 6)(), (C.c_double * 3)()
    assert L.hry_curvature_summary(None, s) == nat.E_ARG and L.hry_curvature_totals(None, t) == nat.E_ARG
    assert L.hry_curvature_stat(None, None, None) == nat.E_ARG
    rows = C.c_uint64()
    assert L.hry_curvature_get(None, b"mean", None, C.byref(rows), None, None) == nat.E_ARG
    L.hry_curvature_free(None)


# ---- the meshes
def hexagon():
    """a flat regular hexagonal patch: the centre, vertex 0, and six neighbours at distance 1"""
    a = 2 * np.pi * np.arange(6) / 6
    pos = np.concatenate([[[0, 0, 0]], np.stack([np.cos(a), np.sin(a), np.zeros(6)], axis=1)]).astype(np.float32)
    tris = np.array([[0, 1 + i, 1 + (i + 1) % 6] for i in range(6)], np.uint32)
    return pos, np.full(6, 3, np.uint8), tris.reshape(-1)


def obtuse_sheet():
    """four triangles about the edge 0 - 1: (0, 1, 2) is obtuse at 2, (0, 3, 1) has acute angles only, (0, 2, 4) and (2, 1, 4) are
    obtuse at 2 again; slightly out of plane"""
    pos = np.float32([[0, 0, 0], [4, 0, 0], [2, 0.5, 0], [2, -3, 0.2], [2, 3, 0.1]])
    return pos, np.full(4, 3, np.uint8), np.array([[0, 1, 2], [0, 3, 1], [0, 2, 4], [2, 1, 4]], np.uint32).reshape(-1)


def euler_of(mesh):
    """V - E + T over the fan triangles and the vertices they name"""
    pos, deg, idx = mesh
    I, _ = sr.fan(deg, idx)
    e = er.build(I, np.arange(len(pos)))
    return len(np.unique(I)) - e["summary"][0] + len(I)


def turns(r):
    return r["totals"][1] / cv.TWO_PI


def gen_arrays(m):
    return np.stack([m.verts["x"], m.verts["y"], m.verts["z"]], axis=1).astype(np.float32), m.degrees, m.indices


# ---- the restatement against closed forms
@pytest.mark.parametrize("cube", [cube_triangles, cube_quads], ids=["triangles", "quads"])
def test_cubes(cube):
    r = cv.of_arrays(*cube())
    d = r["decoded"]
    assert r["summary"] == (8, 8, 0, 0, 0, 0) and (r["vertex_class"] == cv.INTERIOR).all()
    assert (np.abs(d["defect"] - np.pi / 2) <= 4 * ULP * (np.pi / 2)).all(), d["defect"] - np.pi / 2
    assert abs(d["A"].sum() - 6.0) <= 2.0 ** -40 * r["scale"]["totals"][0] and abs(r["totals"][0] - 6.0) <= 2.0 ** -40 * r["scale"]["totals"][0]
    assert abs(turns(r) - 2.0) <= 2.0 ** -40 * r["scale"]["totals"][1] / cv.TWO_PI
    assert (r["gaussian"] > 0).all() and (r["mean"] > 0).all()   # wound outward: convex towards its normals


def test_flat_hexagon():
    r = cv.of_arrays(*hexagon())
    d = r["decoded"]
    assert r["summary"] == (7, 1, 6, 0, 0, 0) and d["class"][0] == cv.INTERIOR and (d["class"][1:] == cv.BOUNDARY).all()
    assert abs(d["defect"][0]) <= 2.0 ** -40 * d["scale_theta"][0]
    assert (np.abs(d["L"][0]) <= 2.0 ** -40 * d["scale_L"][0]).all() and d["scale_L"][0].max() > 1
    # the Voronoi cell of the centre: a hexagon of inradius 1 / 2.  The float32 positions are within 2^-24 of the regular ones, the
    # area within a few 2^-24 of its own
    assert abs(d["A"][0] - np.sqrt(3) / 2) <= 8 * 2.0 ** -24 * np.sqrt(3) / 2
    assert (r["branch"] == 0).all()
    # the rim: flat, so pi less the two angles of 60 degrees
    assert (np.abs(d["defect"][1:] - np.pi / 3) <= 8 * 2.0 ** -24).all()


def test_obtuse_sheet_takes_every_branch():
    r = cv.of_arrays(*obtuse_sheet())
    br = r["branch"].reshape(-1, 3)
    assert sorted(set(br.reshape(-1).tolist())) == [0, 1, 2]
    assert br.tolist() == [[2, 2, 1], [0, 0, 0], [2, 1, 2], [1, 2, 2]]
    share, area = r["slot_area"].reshape(-1, 3), r["tri_area"]
    obtuse = (br != 0).any(axis=1)
    assert np.array_equal(share[obtuse].sum(axis=1), area[obtuse])   # a half and two quarters: exact
    assert np.array_equal(share[br == 1], 0.5 * np.repeat(area, 3).reshape(-1, 3)[br == 1])
    assert np.array_equal(share[br == 2], 0.25 * np.repeat(area, 3).reshape(-1, 3)[br == 2])
    assert (np.abs(share[~obtuse].sum(axis=1) - area[~obtuse]) <= 2.0 ** -40 * np.abs(share[~obtuse]).sum(axis=1)).all()
    assert r["summary"] == (5, 1, 4, 0, 0, 0) and r["vertex_class"][2] == cv.INTERIOR   # vertex 2 lies within the triangle 0 1 4


MESHES = {
    "torus": lambda: gen_arrays(mg.torus(24, 16)),
    "icosphere": lambda: gen_arrays(mg.icosphere(2)),
    "obtuse_sheet": obtuse_sheet,
    "grid": lambda: gen_arrays(mg.grid(9, 8)),
    "torus_holes": lambda: gen_arrays(mg.with_holes(mg.torus(24, 16), 3)),
}


@pytest.mark.parametrize("name", ["torus", "icosphere", "obtuse_sheet"])
def test_vertex_areas_sum_to_the_surface(name):
    r = cv.of_arrays(*MESHES[name]())
    assert r["summary"][5] == 0 and r["summary"][4] == 0
    assert abs(r["totals"][0] - r["tri_area"].sum()) <= 2.0 ** -40 * r["scale"]["totals"][0], (r["totals"][0], r["tri_area"].sum())
    assert abs(r["decoded"]["A"].sum() - r["tri_area"].sum()) <= 2.0 ** -40 * r["scale"]["totals"][0]


@pytest.mark.parametrize("name,euler", [("icosphere", 2), ("torus", 0), ("grid", 1), ("torus_holes", -3)])
def test_gauss_bonnet(name, euler):
    mesh = MESHES[name]()
    r = cv.of_arrays(*mesh)
    assert euler_of(mesh) == euler and r["summary"][3] == 0 and r["summary"][5] == 0
    assert (r["summary"][2] > 0) == (name in ("grid", "torus_holes"))
    assert abs(turns(r) - euler) <= 2.0 ** -40 * r["scale"]["totals"][1] / cv.TWO_PI, turns(r)
    shells = sr.of_mesh(mg.Mesh(util.xyz(mesh[0]), mesh[1], mesh[2]), geometry=False)["shell_counts"]
    assert len(shells) == 1 and sr.euler(shells[0]) == euler


def test_sphere_is_convex_everywhere():
    m = mg.icosphere(3, sigma=0)
    r = cv.of_mesh(m)
    assert (r["vertex_class"] == cv.INTERIOR).all() and (r["mean"] > 0).all() and (r["gaussian"] > 0).all()
    # ... and about a unit sphere's: H = K = 1, area 4 pi (a polyhedron inscribed in it: a little less)
    assert np.abs(r["mean"] - 1).max() < 0.05 and np.abs(r["gaussian"] - 1).max() < 0.1 and 0.97 * 4 * np.pi < r["totals"][0] < 4 * np.pi


def test_classes_and_isolated_vertices():
    # two triangles on one edge, a third on the same edge (three sides: irregular ends), and a vertex no triangle names
    pos = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [0.5, 0.5, 1], [9, 9, 9]])
    r = cv.of_arrays(pos, np.full(3, 3, np.uint8), np.array([[0, 1, 2], [1, 3, 2], [1, 4, 2]], np.uint32).reshape(-1))
    assert r["vertex_class"].tolist() == [2, 3, 3, 2, 2, 8] and r["summary"] == (6, 0, 3, 2, 1, 1)
    for name in cv.FLOATS:
        assert not r[name][5].view(np.uint32).any(), name   # +0 everywhere
    # the totals' rounds: 256 rows and one more are two chunks, then one
    rows = np.random.default_rng(5).random((257, 3))
    want = np.zeros(3)
    for row in rows[:256]:
        want = want + row   # (one after the other; Python's sum() compensates)
    want = (np.zeros(3) + want) + (np.zeros(3) + rows[256])
    assert np.array_equal(cv.fold(rows), want) and np.array_equal(cv.fold(np.zeros((0, 3))), np.zeros(3))
