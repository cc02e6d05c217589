"""Consistent winding per patch of a render build (include/harry_amd.h: hry_orient_build; kernels: harry_amd/csrc/device/orient.hip
and the measures of shells.hip over the patches) against the restatement of tests/orient_ref.py, built from the same run's render
buffers: the plain build and every flag combination.  Integer buffers are compared with array_equal; patch_measures is expected
bit-equal to the float64 restatement rounded once to float32, with one float32 step of slack per value (the shells' slack: a double
sqrt or division that is not correctly rounded); every comparison prints how many values are not bit-equal."""
import ctypes as C
import subprocess
import sys

import numpy as np
import pytest

from harry_amd import _native as nat
from harry_amd import cli
from harry_amd import codec as hc
from harry_amd import meshgen as mg
from harry_amd import objgen as og
from tests import edges_ref as er
from tests import orient_ref as orf
from tests import shells_ref as sr
from tests import util
from tests.util import position_list, same_bytes, xyz

pytestmark = pytest.mark.gpu

COL = {k: i for i, k in enumerate(orf.COLUMNS)}
COMBOS = [(False, False), (True, False), (False, True), (True, True)]   # (majority, outward)


@pytest.fixture(scope="module")
def cx():
    c = hc.Codec(0)
    yield c
    c.close()


def mesh_of(mesh):
    pos, deg, idx = mesh
    return hc.Mesh.from_arrays(xyz(pos), np.asarray(deg, np.uint8), np.asarray(idx, np.uint32))


def gen_arrays(m):
    return np.stack([m.verts["x"], m.verts["y"], m.verts["z"]], axis=1), m.degrees, m.indices


def compare(got, want, label=""):
    for k in orf.FIXED:
        assert got[k].dtype == np.uint32 and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (label, k)
    if "patch_measures" in got:
        assert got["patch_measures"].dtype == np.float32
        differ, steps = er.float_steps(got["patch_measures"], want["patch_measures"])
        print(label, "patch_measures values not bit-equal:", differ, "of", got["patch_measures"].size, "largest distance in float32 steps:", steps)
        assert steps <= 1, (label, differ, steps)


def check(cx, mesh, label="", outward=True):
    """the plain build and every flag combination against the restatement of the same run's render buffers, the summary and the
    stat, and a second build of each for its bytes; returns {(majority, outward): buffers}, the restatement (a function of the two)"""
    rn = cx.render_numpy(mesh)
    want = orf.from_render(rn, mesh.nf, rn[f"list{position_list(mesh)}"][:, :3] if outward else None)
    out = {}
    for maj, outw in COMBOS:
        if outw and not outward:
            continue
        got = cx.orient_numpy(mesh, majority=maj, outward=outw)
        st = cx.orient_stat()
        w = want(maj, outw)
        tag = f"{label} majority={int(maj)} outward={int(outw)}"
        assert sorted(got) == sorted(orf.FIXED + (orf.OUTWARD if outw else ())), tag
        assert st["uploaded_bytes"] == 0 and (st["device_ms"] > 0 or not mesh.ntri)
        assert tuple(st[k] for k in orf.SUMMARY) == w["summary"], (tag, st, w["summary"])
        compare(got, w, tag)
        same_bytes(got, cx.orient_numpy(mesh, majority=maj, outward=outw))
        out[(maj, outw)] = got
    return out, want


def counts(got):
    return got["patch_counts"].astype(np.int64)


# ---- 1. tetrahedra
def test_tetrahedron_wound(cx):
    got, _ = check(cx, mesh_of(orf.tetra()), "tetra")
    for g in got.values():
        assert counts(g).tolist() == [[4, 4, 0, 0, 0, 0, 1, 0]] and not g["tri_flip"].any()
        assert g["oriented_indices"].tolist() == orf.TETRA_TRIS
    assert got[(True, True)]["patch_measures"][0, 1] == np.float32(1 / 6)


def test_tetrahedron_one_turned(cx):
    got, _ = check(cx, mesh_of(orf.turned(orf.tetra(), [0])), "tetra, triangle 0 turned")
    assert got[(False, False)]["tri_flip"].tolist() == [0, 1, 1, 1]                    # relative to the lowest triangle: 3 flips
    assert got[(True, False)]["tri_flip"].tolist() == [1, 0, 0, 0]                     # the smaller side: 1
    assert got[(True, True)]["oriented_indices"].tolist() == orf.TETRA_TRIS
    assert got[(False, True)]["oriented_indices"].tolist() == orf.TETRA_TRIS           # the three put right, then the patch inverted
    assert counts(got[(False, True)])[0].tolist() == [4, 4, 1, 1, 3, 0, 1, 1]


def test_tetrahedron_all_turned(cx):
    got, _ = check(cx, mesh_of(orf.turned(orf.tetra(), [0, 1, 2, 3])), "tetra, all turned")
    for key in ((False, False), (True, False)):
        assert not got[key]["tri_flip"].any() and counts(got[key])[0, COL["inverted"]] == 0
    for key in ((False, True), (True, True)):                                          # only OUTWARD sees it
        assert got[key]["tri_flip"].tolist() == [1] * 4 and counts(got[key])[0].tolist() == [4, 4, 4, 4, 0, 0, 1, 1]
        assert got[key]["patch_measures"][0, 1] == np.float32(1 / 6) and got[key]["oriented_indices"].tolist() == orf.TETRA_TRIS
    assert cx.orient_stat()["inverted"] == 1 and cx.orient_stat()["flipped"] == 4


# ---- 2. strips and closed surfaces
def test_moebius_strip(cx):
    got, _ = check(cx, mesh_of(orf.band(8, twist=True)), "moebius")
    for g in got.values():
        c = counts(g)
        assert c.shape == (1, 8) and c[0, COL["triangles"]] == 16 and c[0, COL["orientable"]] == 0 and not g["tri_flip"].any()
    st = cx.orient_stat()
    assert st["orientable"] == 0 and st["flipped"] == 0 and st["remaining"] == st["against"] > 0


def test_untwisted_strip_with_turns(cx):
    mesh, flags = orf.random_turns(orf.band(8))
    got, _ = check(cx, mesh_of(mesh), "band")
    for g in got.values():
        c = counts(g)[0]
        assert c[COL["orientable"]] == 1 and c[COL["open"]] == 16 and c[COL["inverted"]] == 0 and c[COL["against"]] > 0
    assert np.array_equal(got[(True, True)]["face_flip"] != 0, flags if 2 * flags.sum() <= 16 else ~flags)


def misoriented_of(cx, pos, tris):
    """the shells' misoriented edges of the triangles `tris`, from an edges build of a mesh made from the arrays"""
    m = hc.Mesh.from_arrays(xyz(pos), np.full(len(tris), 3, np.uint8), np.ascontiguousarray(tris, np.uint32).reshape(-1))
    return int(cx.shells_numpy(m)["shell_counts"][:, 6].sum())


@pytest.mark.parametrize("quads", [False, True], ids=["triangles", "quads"])
def test_torus_grid_with_turns(cx, quads):
    mesh, flags = orf.random_turns(orf.closed_grid(quads=quads))
    got, _ = check(cx, mesh_of(mesh), "torus 6 x 6")
    assert misoriented_of(cx, mesh[0], orf.sr.fan(mesh[1], mesh[2])[0]) > 0
    for key, g in got.items():
        assert counts(g)[0, COL["orientable"]] == 1 and counts(g)[0, COL["open"]] == 0
        assert misoriented_of(cx, mesh[0], g["oriented_indices"]) == 0, key
    assert np.array_equal(got[(True, False)]["face_flip"] != 0, flags)


def test_klein_bottle(cx):
    mesh = orf.closed_grid(klein=True)
    got, _ = check(cx, mesh_of(mesh), "klein 6 x 6")
    for g in got.values():
        c = counts(g)
        assert c.shape == (1, 8) and c[0, COL["open"]] == 0 and c[0, COL["orientable"]] == 0 and not g["tri_flip"].any()
    st = cx.orient_stat()
    assert st["remaining"] == st["against"] == misoriented_of(cx, mesh[0], got[(True, True)]["oriented_indices"]) > 0   # nothing to be done


# ---- 3. non-manifold edges join shells, not patches
def test_two_tetrahedra_on_one_edge(cx):
    mesh = orf.turned(orf.two_tetrahedra(), [1, 6])
    m = mesh_of(mesh)
    got, _ = check(cx, m, "two tetrahedra")
    assert len(cx.shells_numpy(m)["shell_first"]) == 1
    g = got[(True, False)]
    assert g["tri_patch"].tolist() == [0] * 4 + [1] * 4 and g["patch_first"].tolist() == [0, 4]
    assert g["face_flip"].tolist() == [0, 1, 0, 0, 0, 0, 1, 0] and counts(g)[:, COL["open"]].tolist() == [2, 2]   # each on its own


def test_three_triangles_on_one_edge(cx):
    got, _ = check(cx, mesh_of(orf.book3()), "book of three")
    for g in got.values():
        assert g["tri_patch"].tolist() == [0, 1, 2] and counts(g)[:, COL["open"]].tolist() == [3, 3, 3] and not g["tri_flip"].any()


# ---- 4. the same-face rule
def test_quad_with_a_four_sided_diagonal(cx):
    got, _ = check(cx, mesh_of(orf.quad_with_fins()), "quad with fins")
    for g in got.values():
        assert g["tri_patch"].tolist() == [0, 0, 1, 2] and counts(g)[0, :2].tolist() == [2, 1] and g["face_flip"].shape == (3,)


def test_mixed_polygons_with_turns(cx):
    clean = gen_arrays(mg.torus(24, 16, polys="mixed"))
    mesh, flags = orf.random_turns(clean)
    got, _ = check(cx, mesh_of(mesh), "mixed polygons")
    g = got[(True, False)]
    assert counts(g).shape == (1, 8) and np.array_equal(g["face_flip"] != 0, flags) and counts(g)[0, COL["flipped_faces"]] == flags.sum()
    assert np.array_equal(orf.flip_faces(mesh[1], mesh[2], g["face_flip"]), clean[2])


# ---- 5. seams and degenerate edges
def test_uv_seams_do_not_cut_patches(cx):
    mesh = hc.Mesh.from_obj(og.scene(mg.torus(24, 26, polys="mixed"), normals="smooth", tex="atlas", charts=5).obj, "")
    got, _ = check(cx, mesh, "atlas")
    assert len(cx.render_numpy(mesh)["vertex_source"]) > mesh.nv                       # the render build has split vertices
    for g in got.values():
        assert counts(g).shape == (1, 8) and counts(g)[0, COL["open"]] == 0 and counts(g)[0, COL["orientable"]] == 1


def test_repeated_vertex(cx):
    got, _ = check(cx, mesh_of(orf.repeated_vertex()), "repeated vertex")
    for g in got.values():
        assert g["tri_patch"].tolist() == [0, 0, 1, 2] and counts(g)[:, COL["open"]].tolist() == [4, 3, 3]


# ---- 6. large meshes: relations that leave a workgroup's triangles in LDS, many workgroups
@pytest.mark.parametrize("order", ["generated", "shuffled"])
@pytest.mark.parametrize("size", [(64, 96), (96, 128)], ids=["12288", "24576"])
def test_large_torus(cx, size, order):
    m = mg.torus(*size)
    pos, deg, idx = gen_arrays(m)
    assert len(deg) == 2 * size[0] * size[1]
    tris = idx.reshape(-1, 3)
    if order == "shuffled":
        tris = tris[np.random.default_rng(23).permutation(len(tris))]
    clean = (pos, deg, np.ascontiguousarray(tris).reshape(-1))
    mesh, flags = orf.random_turns(clean)
    got, _ = check(cx, mesh_of(mesh), f"torus {size} {order}")
    g = got[(True, False)]
    assert counts(g).shape == (1, 8) and counts(g)[0, COL["orientable"]] == 1 and np.array_equal(g["face_flip"] != 0, flags)
    assert np.array_equal(g["oriented_indices"].reshape(-1), clean[2])
    assert counts(got[(True, True)])[0, COL["open"]] == 0


# ---- 6b. both builds run the measures over the same triangles (measures.hip): where the winding stage turns nothing, the patches'
# measures are the shells' bit for bit
@pytest.mark.parametrize("name", ["icosphere", "tori"])
def test_patch_measures_are_shell_measures(cx, name):
    """a closed manifold mesh wound consistently: patches are shells, nothing is turned before the outward stage, which negates the
    volume of a patch it inverts (exactly) and touches nothing else.  icosphere(2): 320 triangles, one 256-triangle chunk seam inside
    one shell; multi_component(3, 8, 6): three shells within and across chunks (wound inwards: all three are inverted)"""
    m = {"icosphere": lambda: mg.icosphere(2), "tori": lambda: mg.multi_component(3, 8, 6)}[name]()
    ref = orf.of_mesh(m)   # (the restatement, on the host: the premise)
    assert not ref["tri_flip"].any() and len(ref["patch_first"]) == len(sr.of_mesh(m, geometry=False)["shell_first"])
    mesh = mesh_of(gen_arrays(m))
    o, s = cx.orient_numpy(mesh, outward=True), cx.shells_numpy(mesh, geometry=True)
    assert cx.orient_stat()["patches"] == cx.shells_stat()["shells"] == len(ref["patch_first"])
    assert np.array_equal(o["tri_patch"], s["tri_shell"]) and np.array_equal(o["patch_first"], s["shell_first"])
    c = counts(o)
    inverted = c[:, COL["inverted"]] != 0
    assert np.array_equal(c[:, COL["flipped"]], np.where(inverted, c[:, COL["triangles"]], 0))   # whole inverted patches, nothing else
    pm, sm = o["patch_measures"].view(np.uint32), s["shell_measures"].view(np.uint32)
    assert pm.shape == sm.shape == (len(c), 8)
    assert np.array_equal(pm[:, 0], sm[:, 0]) and np.array_equal(pm[:, 2:], sm[:, 2:])            # area and box: the same bits
    assert np.array_equal(pm[:, 1] & 0x7fffffff, sm[:, 1] & 0x7fffffff)                            # volume: the same magnitude
    assert np.array_equal((pm[:, 1] ^ sm[:, 1]) >> 31 != 0, inverted)                              # ... the sign: where inverted


# ---- 7. no triangles
def test_no_triangles(cx):
    mesh = hc.Mesh.from_arrays(xyz(np.zeros((3, 3))), np.zeros(0, np.uint8), np.zeros(0, np.uint32))
    for maj, outw in COMBOS:   # (a render build without triangles has no "indices" to restate from: the arrays themselves)
        want = orf.of_arrays(np.zeros((3, 3), np.float32), np.zeros(0, np.uint8), np.zeros(0, np.uint32), majority=maj, outward=outw)
        got = cx.orient_numpy(mesh, majority=maj, outward=outw)
        assert sorted(got) == sorted(orf.FIXED + (orf.OUTWARD if outw else ())) and all(a.shape[0] == 0 for a in got.values())
        assert got["patch_counts"].shape == (0, 8) and got["oriented_indices"].shape == (0, 3)
        assert tuple(cx.orient_stat()[k] for k in orf.SUMMARY) == want["summary"] == (0,) * 6 and cx.orient_stat()["uploaded_bytes"] == 0
        compare(got, want, "no triangles")
        same_bytes(got, cx.orient_numpy(mesh, majority=maj, outward=outw))


# ---- 8. refusals
def raw_build(cx, mesh, render_of, edges_of, flags):
    """hry_orient_build of `mesh` with a render build of `render_of` and an edges build of `edges_of`: (status, handle value, error text)"""
    L = nat.load()
    r, r2, e, o = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(1)
    nat.check(L.hry_render_build(cx.h, render_of.h, C.byref(r)))
    nat.check(L.hry_render_build(cx.h, edges_of.h, C.byref(r2)))
    try:
        nat.check(L.hry_edges_build(cx.h, edges_of.h, r2, 0, C.byref(e)))
        try:
            rc = L.hry_orient_build(cx.h, mesh.h, r, e, flags, C.byref(o))
            text = L.hry_last_error() if rc else b""
            if rc == 0:
                L.hry_orient_free(o)
            return rc, (o.value if rc else None), text
        finally:
            L.hry_edges_free(e)
    finally:
        L.hry_render_free(r)
        L.hry_render_free(r2)


def test_refusals(cx):
    good = mesh_of(orf.tetra())
    other = mesh_of(orf.band(8))
    flat = np.zeros(3, np.dtype([("x", "<f4"), ("y", "<f4")]))
    flat["x"], flat["y"] = [0, 1, 0], [0, 0, 1]
    xy = hc.Mesh.from_arrays(flat, np.array([3], np.uint8), np.array([0, 1, 2], np.uint32))

    def usable():
        assert raw_build(cx, good, good, good, 3)[0] == 0
        assert cx.orient_numpy(good, majority=True, outward=True)["patch_counts"].tolist() == [[4, 4, 0, 0, 0, 0, 1, 0]]

    for flags in (4, 1 | 8, 0x80000000):
        rc, h, text = raw_build(cx, good, good, good, flags)
        assert rc == nat.E_ARG and not h and text
        usable()
    rc, h, text = raw_build(cx, good, other, good, 0)      # a render of another mesh
    assert rc == nat.E_ARG and not h and b"render" in text
    usable()
    rc, h, text = raw_build(cx, good, good, other, 0)      # edges of another mesh
    assert rc == nat.E_ARG and not h and b"edge" in text
    usable()
    for flags in (2, 3):
        rc, h, text = raw_build(cx, xy, xy, xy, flags)     # outward without a z
        assert rc == nat.E_UNSUPPORTED and not h and b"position" in text
        usable()
    assert raw_build(cx, xy, xy, xy, 1)[0] == 0            # ... the flips alone build
    got, _ = check(cx, xy, "xy", outward=False)
    assert counts(got[(True, False)]).tolist() == [[1, 1, 0, 0, 0, 3, 1, 0]]
    with pytest.raises(hc.HryError):
        cx.orient_numpy(xy, outward=True)
    usable()
    L = nat.load()
    r, e = C.c_void_p(), C.c_void_p()
    nat.check(L.hry_render_build(cx.h, good.h, C.byref(r)))
    nat.check(L.hry_edges_build(cx.h, good.h, r, 0, C.byref(e)))
    for args in ((None, good.h, r, e), (cx.h, None, r, e), (cx.h, good.h, None, e), (cx.h, good.h, r, None)):
        o = C.c_void_p(1)
        assert L.hry_orient_build(*args, 0, C.byref(o)) == nat.E_ARG and not o.value
    assert L.hry_orient_build(cx.h, good.h, r, e, 0, None) == nat.E_ARG
    L.hry_edges_free(e)
    L.hry_render_free(r)
    usable()


def test_handle_outlives_inputs_and_get(cx):
    """the handle owns its memory (render and edges are freed before any buffer is read), and hry_orient_get describes the buffers"""
    mesh = mesh_of(orf.turned(orf.two_tetrahedra(), [1]))
    L = nat.load()
    r, e, o = C.c_void_p(), C.c_void_p(), C.c_void_p()
    nat.check(L.hry_render_build(cx.h, mesh.h, C.byref(r)))
    nat.check(L.hry_edges_build(cx.h, mesh.h, r, 0, C.byref(e)))
    nat.check(L.hry_orient_build(cx.h, mesh.h, r, e, 3, C.byref(o)))
    L.hry_edges_free(e)
    L.hry_render_free(r)
    try:
        P, T = L.hry_orient_count(o), mesh.ntri
        assert P == 2
        shapes = {"tri_patch": (T, 1, 4), "tri_flip": (T, 1, 4), "face_flip": (mesh.nf, 1, 4), "oriented_indices": (T, 3, 4), "patch_first": (P, 1, 4),
                  "patch_counts": (P, 8, 4), "patch_measures": (P, 8, 0), "no_such": (0, 0, 0)}
        for name, want in shapes.items():
            dev, rows, width, typ = C.c_void_p(), C.c_uint64(), C.c_int(), C.c_int()
            nat.check(L.hry_orient_get(o, name.encode(), C.byref(dev), C.byref(rows), C.byref(width), C.byref(typ)))
            assert (rows.value, width.value, typ.value) == want and bool(dev.value) == (name != "no_such"), name
        flip = np.empty(T, np.uint32)
        nat.check(L.hry_orient_copy(cx.h, o, b"tri_flip", flip.ctypes.data, 0))
        assert flip.tolist() == [0, 1, 0, 0, 0, 0, 0, 0]
        assert L.hry_orient_copy(cx.h, o, b"no_such", flip.ctypes.data, 0) == nat.E_ARG
        t = (C.c_uint64 * 6)()
        nat.check(L.hry_orient_summary(o, t))
        assert list(t) == [2, 2, 1, 0, 2, 0]
        d, up = C.c_double(), C.c_uint64(7)
        nat.check(L.hry_orient_stat(o, C.byref(d), C.byref(up)))
        assert d.value > 0 and up.value == 0
    finally:
        L.hry_orient_free(o)


# ---- 9. the round trip: orient, flip, encode
def cyclic_triples(tris, tri_face, nf):
    """per face the sorted list of its triangles, each rotated to start at its smallest corner"""
    out = [[] for _ in range(nf)]
    for t, f in zip(np.asarray(tris).reshape(-1, 3).tolist(), tri_face.tolist()):
        k = t.index(min(t))
        out[f].append(tuple(t[k:] + t[:k]))
    return [sorted(x) for x in out]


@pytest.mark.parametrize("polys", ["tri", "quad"])
def test_round_trip(cx, polys):
    x = gen_arrays(mg.torus(24, 16, polys=polys))
    assert set(x[1].tolist()) == ({3} if polys == "tri" else {4})
    y, flags = orf.random_turns(x)
    X, Y = mesh_of(x), mesh_of(y)
    o = cx.orient_numpy(Y, majority=True)
    assert np.array_equal(o["face_flip"] != 0, flags)
    Z = Y.flip_faces(o["face_flip"])
    assert np.array_equal(Z.org(), X.org()) and np.array_equal(Z.face_offsets(), X.face_offsets())
    assert np.array_equal(np.array(Z.list_data(1)), np.array(X.list_data(1)))
    bx, by, bz = cx.write_hry(X), cx.write_hry(Y), cx.write_hry(Z)
    print(polys, "bytes: wound", len(bx), "turned", len(by), "oriented", len(bz))
    assert bz == bx and len(bx) < len(by)
    rz = cx.render_numpy(Z)
    if polys == "tri":
        assert np.array_equal(rz["indices"], o["oriented_indices"])
    else:   # the fan order inside a turned face reverses
        assert not np.array_equal(rz["indices"], o["oriented_indices"])
        assert cyclic_triples(rz["indices"], rz["tri_face"], Z.nf) == cyclic_triples(o["oriented_indices"], cx.render_numpy(Y)["tri_face"], Y.nf)
    torch = pytest.importorskip("torch")
    assert np.array_equal(np.array(Y.flip_faces(torch.from_numpy(o["face_flip"].astype(np.int32))).org()), np.array(X.org()))


# ---- 10. the command line
def run_cli(*args):
    r = subprocess.run([cli.HARRY] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def orientation_line(out):
    lines = [l.split() for l in out.splitlines() if l.startswith("Orientation:")]
    assert len(lines) == 1 and tuple(lines[0][1::2]) == orf.SUMMARY, out
    return tuple(map(int, lines[0][2::2]))


def test_orient_option(cx, tmp_path):
    x = gen_arrays(mg.torus(24, 16))
    y, flags = orf.random_turns(x)
    (tmp_path / "x.ply").write_bytes(mesh_of(x).to_ply())
    (tmp_path / "y.ply").write_bytes(mesh_of(y).to_ply())
    want = orf.of_arrays(*y, majority=True)["summary"]
    out = run_cli(tmp_path / "y.ply", "--orient")
    assert orientation_line(out) == want and want[2] == flags.sum() and "Writing output" not in out
    out = run_cli(tmp_path / "y.ply", tmp_path / "y.hry", "--orient", "--shells", "--topology")
    marked = [l.split(":")[0] for l in out.splitlines() if l.startswith(("Topology:", "Shells:", "Shell:", "Orientation:"))]
    assert marked == ["Topology", "Shells", "Shell", "Orientation"] and orientation_line(out) == want
    shells = [l.split() for l in out.splitlines() if l.startswith("Shells:")][0]
    assert int(shells[shells.index("misoriented") + 1]) == 1                            # those lines describe the source mesh
    run_cli(tmp_path / "x.ply", tmp_path / "plain.hry")
    dec, ref = cx.read_hry((tmp_path / "y.hry").read_bytes()), cx.read_hry((tmp_path / "plain.hry").read_bytes())
    assert np.array_equal(dec.org(), ref.org()) and np.array_equal(np.array(dec.list_data(1)), np.array(ref.list_data(1)))
    assert (tmp_path / "y.hry").read_bytes() == (tmp_path / "plain.hry").read_bytes()
    out = run_cli(tmp_path / "x.ply", tmp_path / "x.hry", "--orient")                   # nothing to flip: the same container
    assert orientation_line(out)[2] == 0 and (tmp_path / "x.hry").read_bytes() == (tmp_path / "plain.hry").read_bytes()
    cube = [[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]]
    inward = [[0, 1, 2, 3], [4, 7, 6, 5], [0, 4, 5, 1], [1, 5, 6, 2], [2, 6, 7, 3], [3, 7, 4, 0]]   # clockwise seen from outside
    (tmp_path / "cube.ply").write_bytes(mesh_of((cube, [4] * 6, np.array(inward).reshape(-1))).to_ply())
    assert orientation_line(run_cli(tmp_path / "cube.ply", "--orient")) == (1, 1, 0, 0, 0, 0)
    assert orientation_line(run_cli(tmp_path / "cube.ply", "--orient-outward")) == (1, 1, 12, 1, 0, 0)
    out = run_cli(tmp_path / "cube.ply", tmp_path / "cube.hry", "--orient-outward")
    turned = cx.read_hry((tmp_path / "cube.hry").read_bytes())
    assert orientation_line(run_cli(tmp_path / "cube.hry", "--orient-outward")) == (1, 1, 0, 0, 0, 0)
    assert turned.nf == 6 and cx.orient_numpy(turned, outward=True)["patch_measures"][0, 1] == 1.0


# ---- 11. torch: Codec.orient
TORCH_CHILD = r"""
import sys
import numpy as np
import torch
torch.cuda.init()   # a PyTorch program: torch holds the device before the codec starts
sys.path.insert(0, sys.argv[1])
from harry_amd import codec as hc
from harry_amd import meshgen as mg
from tests import orient_ref as orf
m = mg.torus(24, 16, polys="mixed")
mesh_arrays, flags = orf.random_turns((np.stack([m.verts["x"], m.verts["y"], m.verts["z"]], axis=1), m.degrees, m.indices))
v = np.zeros(len(m.verts), np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4")]))
v["x"], v["y"], v["z"] = mesh_arrays[0].T
mesh = hc.Mesh.from_arrays(v, m.degrees, mesh_arrays[2])
c = hc.Codec(0)
ref = c.orient_numpy(mesh, majority=True, outward=True)
got = c.orient(mesh, majority=True, outward=True)
assert sorted(got) == sorted(ref)
for k, t in got.items():
    assert t.device == torch.device("cuda", 0) and t.dtype == (torch.float32 if ref[k].dtype == np.float32 else torch.int32), k
    assert tuple(t.shape) == ref[k].shape and np.array_equal(t.cpu().numpy().view(np.uint8), ref[k].view(np.uint8)), k
assert sorted(c.orient(mesh)) == sorted(c.orient_numpy(mesh)) and "patch_measures" not in c.orient(mesh)
plain = c.orient(mesh, majority=True)
st = c.orient_stat()
assert st["patches"] == 1 and st["orientable"] == 1 and st["uploaded_bytes"] == 0 and st["flipped"] == int(plain["tri_flip"].sum())
assert np.array_equal(plain["face_flip"].cpu().numpy() != 0, flags)
fixed = mesh.flip_faces(plain["face_flip"])
assert np.array_equal(np.array(fixed.org()), m.indices)
c.close()
print("torch ok")
"""


def test_torch_tensors():
    pytest.importorskip("torch")
    r = subprocess.run([sys.executable, "-c", TORCH_CHILD, util.ROOT], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "torch ok" in r.stdout, r.stdout + r.stderr
