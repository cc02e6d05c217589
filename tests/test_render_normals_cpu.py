"""Normals of a render build (include/harry_amd.h: hry_render_build_ex), the parts that need no GPU: the entry point exists and
refuses null arguments, and the tests' restatement (tests/normals_ref.py) is right on cases with a known answer -- which pins what
the GPU test compares the kernels against."""
import ctypes as C

import numpy as np
import pytest

from harry_amd import _native as nat
from harry_amd import meshgen as mg
from tests import normals_ref as nr


def test_render_build_ex_exported():
    L = nat.load()
    assert hasattr(L, "hry_render_build_ex")
    r = C.c_void_p(1)
    assert L.hry_render_build_ex(None, None, 3, C.byref(r)) == nat.E_ARG
    assert not r.value


CUBE_POS = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float32)   # vertex 4x + 2y + z
CUBE_QUADS = np.array([[0, 1, 3, 2], [4, 6, 7, 5], [0, 4, 5, 1], [2, 3, 7, 6], [0, 2, 6, 4], [1, 5, 7, 3]], np.uint32)   # outward


@pytest.mark.parametrize("mode", ["area", "angle"])
def test_unit_cube(mode):
    fn, vn, guard = nr.normals(CUBE_POS, np.full(6, 4, np.uint8), CUBE_QUADS.reshape(-1), mode)
    want_f = np.array([[-1, 0, 0], [1, 0, 0], [0, -1, 0], [0, 1, 0], [0, 0, -1], [0, 0, 1]], np.float32)
    assert np.array_equal(fn, want_f)
    want_v = (2.0 * CUBE_POS.astype(np.float64) - 1.0) / np.sqrt(3.0)
    assert guard.all()
    assert np.abs(vn.astype(np.float64) - want_v).max() <= nr.TOL


def test_translation_does_not_cancel():
    """the cross products are taken relative to corner 0: far from the origin the face normals of the cube stay exact"""
    fn, _, _ = nr.normals(CUBE_POS + np.float32(65536.0), np.full(6, 4, np.uint8), CUBE_QUADS.reshape(-1))
    assert np.array_equal(np.abs(fn).sum(axis=1), np.ones(6, np.float32))


@pytest.mark.parametrize("mode", ["area", "angle"])
def test_torus_against_stored_normals(mode):
    """a sanity check of the restatement, not of a kernel: on a fine torus without noise the vertex normals lie within the angle
    one cell subtends (2 pi / 48 < 0.14 rad: cos > 0.99) of the analytic ones the generator stores -- up to one sign for the whole
    mesh: the generator winds its faces clockwise seen from outside, so the computed normals point into the tube"""
    m = mg.torus(64, 48, normals=True, sigma=0)
    _, vn, guard = nr.of_mesh(m, mode)
    stored = np.stack([m.verts[k] for k in ("nx", "ny", "nz")], axis=1).astype(np.float64)
    assert guard.all()
    assert (-np.sum(vn.astype(np.float64) * stored, axis=1) > 0.99).all()


def test_degenerate_faces_and_isolated_vertex():
    pos = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0], [4, 0, 0], [7, 7, 7]], np.float32)
    # a good triangle, a repeated index, three collinear corners; vertex 4 is unreferenced
    fn, vn, _ = nr.normals(pos, np.full(3, 3, np.uint8), np.array([0, 1, 2, 0, 1, 1, 0, 1, 3], np.uint32))
    assert np.array_equal(fn, np.array([[0, 0, 1], [0, 0, 0], [0, 0, 0]], np.float32))
    assert np.array_equal(vn, np.array([[0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, 0], [0, 0, 0]], np.float32))


def test_order_of_the_sum_moves_at_most_one_step():
    """summing a vertex's corners in another order moves no float32 component of the GPU test's inputs by more than one step: the
    tolerance of normals_ref covers the hubs' other association"""
    m = mg.torus(24, 16)
    _, vn, guard = nr.of_mesh(m, "area")
    rng = np.random.default_rng(1)
    perm = rng.permutation(m.nf)
    idx = m.indices.reshape(-1, 3)[perm].reshape(-1)
    _, vn2, _ = nr.normals(nr.positions_of(m.verts), m.degrees, idx, "area")
    assert guard.all()
    assert np.abs(vn.astype(np.float64) - vn2.astype(np.float64)).max() <= nr.TOL
