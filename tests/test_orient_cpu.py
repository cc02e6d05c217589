"""What of the orientation needs no GPU: hry_mesh_flip_faces (include/harry_amd.h; harry_amd/csrc/host/flip_faces.cpp) on the host
meshes, and the restatement of hry_orient_build (tests/orient_ref.py) pinned on the designed meshes the GPU tests build."""
import ctypes as C

import numpy as np
import pytest

from harry_amd import _native as nat
from harry_amd import codec as hc
from harry_amd import meshgen as mg
from harry_amd import objgen as og
from tests import orient_ref as orf

COL = {k: i for i, k in enumerate(orf.COLUMNS)}


def xyz(pos):
    v = np.zeros(len(pos), np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4")]))
    v["x"], v["y"], v["z"] = np.asarray(pos, np.float32).T
    return v


def host_mesh(mesh):
    pos, deg, idx = mesh
    return hc.Mesh.from_arrays(xyz(pos), deg, idx)


def test_entry_points():
    L = nat.load()
    for name in ("build", "count", "get", "copy", "summary", "stat", "free"):
        assert hasattr(L, "hry_orient_" + name), name
    assert hasattr(L, "hry_mesh_flip_faces") and L.hry_abi_version() == 6
    assert (nat.ORIENT_MAJORITY, nat.ORIENT_OUTWARD) == (1, 2)


# ---- hry_mesh_flip_faces
def arrays(m):
    out = {"face_offsets": m.face_offsets().copy(), "org": m.org().copy()}
    for l in range(m.nlists):
        out[f"list{l}"] = np.array(m.list_data(l)).copy()
    if m.general:
        for kind in range(3):
            out[f"bind{kind}"] = np.array(m.bindings(kind)).copy()
    return out


def flip_cases():
    tri = mg.torus(12, 10)
    mixed = mg.torus(12, 10, polys="mixed")
    return {
        "triangles": lambda: hc.Mesh.from_ply(tri.to_ply()),
        "mixed": lambda: hc.Mesh.from_arrays(mixed.verts, mixed.degrees, mixed.indices),
        "obj": lambda: hc.Mesh.from_obj(og.scene(mg.torus(12, 10, polys="mixed"), normals="smooth", tex="atlas", charts=3).obj, ""),
    }


@pytest.mark.parametrize("name", ["triangles", "mixed", "obj"])
def test_flip_is_an_involution_and_corners_keep_their_records(name):
    m = flip_cases()[name]()
    before = arrays(m)
    flags = np.random.default_rng(3).random(m.nf) < 0.4
    assert flags.any() and not flags.all()
    once = m.flip_faces(flags)
    a = arrays(once)
    off = before["face_offsets"].astype(np.int64)
    deg = np.diff(off)
    assert np.array_equal(a["face_offsets"], before["face_offsets"]) and once.nv == m.nv and once.general == m.general
    assert np.array_equal(a["org"], orf.flip_faces(deg, before["org"], flags)) and not np.array_equal(a["org"], before["org"])
    for k in before:
        if k.startswith("list") or k in ("bind0", "bind1"):
            assert np.array_equal(a[k], before[k]), k                  # records, faces' and vertices' bindings: untouched
    if m.general:
        rows = before["bind2"].reshape(m.ne, -1)
        assert rows.shape[1] > 0 and len(np.unique(rows, axis=0)) > m.nv   # corners do name records of their own
        # corner j of a turned face is corner k - j of the source: its vertex and its record rows arrive together
        source = orf.flip_faces(deg, np.arange(m.ne), flags)
        assert np.array_equal(a["org"], before["org"][source]) and np.array_equal(a["bind2"].reshape(m.ne, -1), rows[source])
    twice = once.flip_faces(flags)
    b = arrays(twice)
    assert sorted(b) == sorted(before) and all(np.array_equal(b[k], before[k]) for k in before)
    assert np.array_equal(arrays(m)["org"], before["org"])             # the source is left alone
    none = m.flip_faces(np.zeros(m.nf, np.uint32))
    assert all(np.array_equal(arrays(none)[k], before[k]) for k in before)


def borders(m):
    """the edges with a half-edge that found no twin (a turned neighbour leaves both half-edges of the edge without one)"""
    h = np.flatnonzero(m.twin() == np.arange(m.ne))
    org = m.org().astype(np.int64)
    off = m.face_offsets().astype(np.int64)
    face = np.searchsorted(off, h, side="right") - 1
    nxt = np.where(h + 1 == off[face + 1], off[face], h + 1)
    return len({(min(a, b), max(a, b)) for a, b in zip(org[h], org[nxt])})


def test_one_turned_face_of_a_tetrahedron_is_three_more_borders():
    m = host_mesh(orf.tetra())
    assert borders(m) == 0
    t = m.flip_faces([0, 0, 1, 0])
    assert borders(t) == 3 and borders(m) == 0 and int((t.twin() == np.arange(12)).sum()) == 6   # both sides of each of the three
    assert t.org().reshape(-1, 3).tolist() == [[0, 2, 1], [0, 1, 3], [0, 2, 3], [1, 2, 3]]
    assert borders(t.flip_faces([0, 0, 1, 0])) == 0
    assert borders(m.flip_faces([1, 1, 1, 1])) == 0                    # all turned: consistent again


def test_flip_refusals():
    L = nat.load()
    m = host_mesh(orf.tetra())
    flags = np.zeros(4, np.uint32)
    for args in ((None, flags.ctypes.data), (m.h, None)):
        out = C.c_void_p(1)
        assert L.hry_mesh_flip_faces(*args, C.byref(out)) == nat.E_ARG and not out.value
    assert L.hry_mesh_flip_faces(m.h, flags.ctypes.data, None) == nat.E_ARG
    with pytest.raises(hc.HryError):
        m.flip_faces(np.zeros(3, np.uint32))                           # one value per face
    out = C.c_void_p()
    assert L.hry_mesh_flip_faces(m.h, flags.ctypes.data, C.byref(out)) == 0 and out.value
    L.hry_mesh_free(out)


# ---- the restatement on the designed meshes
def test_tetrahedra():
    r = orf.of_arrays(*orf.tetra(), outward=True)
    assert r["summary"] == (1, 1, 0, 0, 0, 0) and r["patch_counts"].tolist() == [[4, 4, 0, 0, 0, 0, 1, 0]]
    assert r["patch_measures"][0, 1] == np.float32(1 / 6) and r["patch_measures"][0, 2:].tolist() == [0, 0, 0, 1, 1, 1]
    one = orf.turned(orf.tetra(), [0])
    r = orf.of_arrays(*one)
    assert r["tri_flip"].tolist() == [0, 1, 1, 1] and r["summary"] == (1, 1, 3, 0, 3, 0)   # relative to the lowest triangle
    r = orf.of_arrays(*one, majority=True)
    assert r["tri_flip"].tolist() == [1, 0, 0, 0] and r["oriented_indices"].tolist() == orf.TETRA_TRIS
    every = orf.turned(orf.tetra(), [0, 1, 2, 3])
    for kw in ({}, {"majority": True}):
        assert orf.of_arrays(*every, **kw)["summary"] == (1, 1, 0, 0, 0, 0)
    for kw in ({"outward": True}, {"majority": True, "outward": True}):
        r = orf.of_arrays(*every, **kw)
        assert r["summary"] == (1, 1, 4, 1, 0, 0) and r["patch_counts"].tolist() == [[4, 4, 4, 4, 0, 0, 1, 1]]
        assert r["oriented_indices"].tolist() == orf.TETRA_TRIS and r["patch_measures"][0, 1] == np.float32(1 / 6)
    two = orf.turned(orf.tetra(), [0, 1])                              # a tie: the lowest triangle keeps its winding
    assert orf.of_arrays(*two, majority=True)["tri_flip"].tolist() == [0, 0, 1, 1]


def test_moebius_and_band():
    r = orf.of_arrays(*orf.band(8, twist=True), majority=True, outward=True)
    c = r["patch_counts"][0]
    assert len(r["patch_counts"]) == 1 and c[COL["triangles"]] == 16 and c[COL["orientable"]] == 0 and c[COL["open"]] == 16
    assert not r["tri_flip"].any() and r["summary"][4] == r["summary"][5] > 0
    mesh, flags = orf.random_turns(orf.band(8))
    r = orf.of_arrays(*mesh, majority=True, outward=True)
    c = r["patch_counts"][0]
    assert c[COL["orientable"]] == 1 and c[COL["open"]] == 16 and c[COL["inverted"]] == 0 and c[COL["against"]] > 0
    want = flags if 2 * flags.sum() <= 16 else ~flags
    assert np.array_equal(r["face_flip"], want) and r["summary"][5] == 0


def misoriented(pos, deg, idx):
    from tests import shells_ref as sr
    return int(sr.of_mesh(type("M", (), {"verts": xyz(pos), "degrees": deg, "indices": idx}), geometry=False)["shell_counts"][:, 6].sum())


def test_klein_bottle_and_torus():
    r = orf.of_arrays(*orf.closed_grid(klein=True), majority=True, outward=True)
    c = r["patch_counts"]
    assert c.shape == (1, 8) and c[0, COL["triangles"]] == 72 and c[0, COL["open"]] == 0 and c[0, COL["orientable"]] == 0   # closed, one patch
    assert r["summary"][:4] == (1, 0, 0, 0) and r["summary"][4] == r["summary"][5] > 0
    for quads in (False, True):
        clean = orf.closed_grid(quads=quads)
        assert misoriented(*clean) == 0
        mesh, flags = orf.random_turns(clean)
        assert misoriented(*mesh) > 0
        r = orf.of_arrays(*mesh, majority=True)
        assert r["summary"][:2] == (1, 1) and np.array_equal(r["face_flip"], flags) and r["patch_counts"][0, COL["faces"]] == len(flags)
        fixed = orf.flip_faces(mesh[1], mesh[2], r["face_flip"])
        assert np.array_equal(fixed, clean[2]) and misoriented(mesh[0], mesh[1], fixed) == 0
        # the quads' fan order reverses inside a turned face: the same triangles as cyclic triples, face by face
        assert misoriented(mesh[0], np.full(len(r["oriented_indices"]), 3, np.uint8), r["oriented_indices"].reshape(-1)) == 0


def test_nonmanifold_edges_join_shells_but_not_patches():
    from tests import shells_ref as sr
    pos, deg, idx = orf.turned(orf.two_tetrahedra(), [1, 6])
    r = orf.of_arrays(pos, deg, idx, majority=True)
    assert r["tri_patch"].tolist() == [0] * 4 + [1] * 4 and r["face_flip"].tolist() == [0, 1, 0, 0, 0, 0, 1, 0]
    assert r["patch_counts"][:, COL["open"]].tolist() == [2, 2] and r["patch_first"].tolist() == [0, 4]
    s = sr.of_mesh(type("M", (), {"verts": xyz(pos), "degrees": deg, "indices": idx}), geometry=False)
    assert len(s["shell_first"]) == 1
    r = orf.of_arrays(*orf.book3())
    assert r["tri_patch"].tolist() == [0, 1, 2] and r["patch_counts"][:, COL["open"]].tolist() == [3, 3, 3] and r["summary"][4] == 0


def test_same_face_rule_and_degenerate_edges():
    r = orf.of_arrays(*orf.quad_with_fins())
    assert r["tri_patch"].tolist() == [0, 0, 1, 2] and r["patch_counts"][0, :2].tolist() == [2, 1] and len(r["face_flip"]) == 3
    r = orf.of_arrays(*orf.repeated_vertex())
    assert r["tri_patch"].tolist() == [0, 0, 1, 2] and r["patch_counts"][:, COL["open"]].tolist() == [4, 3, 3]
    m = mg.torus(12, 10, polys="mixed")
    clean = (np.stack([m.verts["x"], m.verts["y"], m.verts["z"]], axis=1), m.degrees, m.indices)
    mesh, flags = orf.random_turns(clean)
    r = orf.of_arrays(*mesh, majority=True)
    assert r["summary"][:2] == (1, 1) and np.array_equal(r["face_flip"], flags)
    assert np.array_equal(orf.flip_faces(mesh[1], mesh[2], r["face_flip"]), clean[2])


def test_no_triangles():
    r = orf.of_arrays(np.zeros((3, 3), np.float32), np.zeros(0, np.uint8), np.zeros(0, np.uint32), majority=True, outward=True)
    assert r["summary"] == (0,) * 6 and r["patch_counts"].shape == (0, 8) and r["patch_measures"].shape == (0, 8)
    assert all(len(r[k]) == 0 for k in orf.FIXED)
