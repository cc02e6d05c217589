"""Shells of a render build (include/harry_amd.h: hry_shells_build; kernels: harry_amd/csrc/device/shells.hip and the ShellVertexKey
numbering of dedup.hip) against the numpy restatement of tests/shells_ref.py, built from the same run's render buffers.  Integer
buffers are compared with array_equal; shell_measures is expected bit-equal to the float64 restatement rounded once to float32, with
one float32 step of slack per value (a double sqrt or division that is not correctly rounded); every comparison prints how many
values are not bit-equal."""
import ctypes as C
import os
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
from tests import seam_meshes as sm
from tests import shells_ref as sr
from tests import util
from tests.util import position_list, same_bytes, xyz_mesh

pytestmark = pytest.mark.gpu

GOLD = os.path.join(util.ROOT, "tests", "golden")
COL = {k: i for i, k in enumerate(sr.COLUMNS)}
SUMMARY = ("shells", "closed", "nonmanifold", "misoriented", "loops", "largest")


@pytest.fixture(scope="module")
def cx():
    c = hc.Codec(0)
    yield c
    c.close()


def mesh_of(m):
    return hc.Mesh.from_arrays(m.verts, m.degrees, m.indices)


def restated(cx, mesh, geometry=True):
    rn = cx.render_numpy(mesh)
    return sr.from_render(rn, mesh.nf, rn[f"list{position_list(mesh)}"][:, :3] if geometry else None, geometry)


def compare(got, want, label=""):
    for k in sr.FIXED:
        assert got[k].dtype == np.uint32 and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k
    if "shell_measures" in got:
        assert got["shell_measures"].dtype == np.float32
        differ, steps = er.float_steps(got["shell_measures"], want["shell_measures"])
        print(label, "shell_measures values not bit-equal:", differ, "of", got["shell_measures"].size, "largest distance in float32 steps:", steps)
        assert steps <= 1, (differ, steps)


def check(cx, mesh, label="", geometry=True):
    """both builds against the restatement, the summary and the stat; returns (buffers, restatement)"""
    want = restated(cx, mesh, geometry)
    plain = cx.shells_numpy(mesh)
    st = cx.shells_stat()
    assert sorted(plain) == sorted(sr.FIXED) and st["uploaded_bytes"] == 0 and st["device_ms"] > 0
    assert tuple(st[k] for k in SUMMARY) == want["summary"], (st, want["summary"])
    compare(plain, want, label)
    if not geometry:
        return plain, want
    got = cx.shells_numpy(mesh, geometry=True)
    assert sorted(got) == sorted(sr.FIXED + sr.GEOMETRY) and tuple(cx.shells_stat()[k] for k in SUMMARY) == want["summary"]
    compare(got, want, label)
    return got, want


# ---- 1. the generator's meshes (their expectations are pinned on the restatement by tests/test_shells_cpu.py)
MESHES = {
    "torus_tri": (lambda: mg.torus(24, 16), dict(S=1, euler=[0], loops=[0])),
    "torus_mixed": (lambda: mg.torus(24, 16, polys="mixed"), dict(S=1, euler=[0], loops=[0])),
    "grid_quads": (lambda: mg.grid(9, 8, quads=True), dict(S=1, euler=[1], loops=[1], boundary=[30])),
    "icosphere": (lambda: mg.icosphere(2), dict(S=1, euler=[2])),
    "nonmanifold": (lambda: mg.with_nonmanifold(mg.torus(12, 10)), dict(S=2, loops=[2, 1], boundary=[4, 3])),
    "soup": (lambda: mg.soup(), dict(S=39, largest=25)),
    "multi": (lambda: mg.multi_component(3, 8, 6), dict(S=3, euler=[0, 0, 0])),
    "holes": (lambda: mg.with_holes(mg.torus(24, 16), 5), dict(S=1, euler=[-5], loops=[4], boundary=[15])),
    "hub_discs": (lambda: mg.hub_discs([5, 7, 40]), dict(S=3, euler=[1, 1, 1], loops=[1, 1, 1])),
    "ribbon": (lambda: mg.ribbon(30), dict(S=1, euler=[0], loops=[2])),
    "ribbon_open": (lambda: mg.ribbon(30, closed=False), dict(S=1, euler=[1], loops=[1])),
}


@pytest.mark.parametrize("name", sorted(MESHES))
def test_against_restatement(cx, name):
    make, expect = MESHES[name]
    got, _ = check(cx, mesh_of(make()), name)
    c = got["shell_counts"]
    assert len(c) == expect["S"] and got["tri_shell"][0] == 0 and (np.diff(got["shell_first"].astype(np.int64)) > 0).all()
    if "euler" in expect:
        assert [sr.euler(r) for r in c] == expect["euler"]
    for k in ("loops", "boundary"):
        if k in expect:
            assert c[:, COL[k]].tolist() == expect[k], k
    if "largest" in expect:
        assert cx.shells_stat()["largest"] == expect["largest"] == c[:, 0].max()
    if name == "torus_mixed":
        assert c[0, :2].tolist() == [768, 584]
    if name == "soup":
        assert (c[:, COL["misoriented"]] > 0).sum() > 1


# ---- 2. strips either side of a wavefront, a block, a chunk and two chunks; whole, and in pieces
def strip(ntri, drop=0, reverse=False, at=0.0):
    """the first ntri triangles of a two-row grid; drop: every drop-th triangle is left out, so the strip falls into pieces"""
    m = mg.grid(ntri // 2 + 2, 2)
    tris = m.indices.reshape(-1, 3)[:ntri]
    assert len(tris) == ntri
    if drop:
        tris = tris[np.arange(ntri) % drop != drop - 1]
    if reverse:
        tris = tris[::-1]
    pos = np.stack([m.verts["x"] + at, m.verts["y"], m.verts["z"]], axis=1)
    return pos, tris


@pytest.mark.parametrize("ntri", [63, 64, 65, 255, 256, 257, 511, 513])
def test_strips(cx, ntri):
    got, _ = check(cx, xyz_mesh(*strip(ntri)), f"strip{ntri}")
    assert len(got["shell_first"]) == 1 and got["shell_counts"][0, 0] == ntri and got["shell_counts"][0, COL["loops"]] == 1
    got, _ = check(cx, xyz_mesh(*strip(ntri, drop=8)), f"strip{ntri}/8")
    assert len(got["shell_first"]) == (ntri + 7) // 8 and got["shell_counts"][:, 0].sum() == ntri - ntri // 8   # runs of seven triangles


def test_interleaved_strips(cx):
    """two strips whose triangles alternate: every chunk holds both shells, each shell spans three chunks"""
    pa, ta = strip(300)
    pb, tb = strip(300, at=50.0)
    tris = np.stack([ta, tb + len(pa)], axis=1).reshape(-1, 3)
    got, want = check(cx, xyz_mesh(np.concatenate([pa, pb]), tris), "interleaved")
    assert np.array_equal(got["tri_shell"], np.arange(600) % 2) and got["shell_first"].tolist() == [0, 1]
    assert got["shell_measures"][0, 0] > 0 and got["shell_measures"][1, 2] >= 50


@pytest.mark.parametrize("order", ["shuffled", "reversed"])
def test_torus_out_of_order(cx, order):
    m = mg.torus(40, 30)
    tris = m.indices.reshape(-1, 3)
    tris = tris[np.random.default_rng(17).permutation(len(tris))] if order == "shuffled" else tris[::-1]
    got, _ = check(cx, hc.Mesh.from_arrays(m.verts, m.degrees, np.ascontiguousarray(tris).reshape(-1)), order)
    assert len(got["shell_first"]) == 1 and sr.euler(got["shell_counts"][0]) == 0 and sr.genus(got["shell_counts"][0]) == 1


@pytest.mark.parametrize("reverse", [False, True], ids=["ascending", "descending"])
def test_long_strip(cx, reverse):
    got, _ = check(cx, xyz_mesh(*strip(4096, reverse=reverse)), "strip4096")
    assert got["shell_counts"].tolist() == [[4096, 4096, 4098, 8193, 4098, 0, 0, 1]]


def book(pages):
    """`pages` triangles round one shared edge, with a strip of ordinary triangles behind them (the edges test's hub)"""
    pos, _, idx = sm.book(pages)
    return xyz_mesh(pos, idx)


def test_book(cx):
    got, _ = check(cx, book(300), "book300")
    c = got["shell_counts"]
    assert len(c) == 2 and c[0, 0] == 300 and c[0, COL["nonmanifold"]] == 1 and c[0, COL["boundary"]] == 600 and c[0, COL["loops"]] == 1
    assert sr.genus(c[0]) is None and cx.shells_stat()["nonmanifold"] == 1


def test_many_chunks_one_shell(cx):
    """more than 32 chunks of one shell: the workgroup path of the ordered sum (and a second, small shell beside it)"""
    pa, ta = strip(40 * 256 + 5)
    pb, tb = strip(7, at=9000.0)
    got, _ = check(cx, xyz_mesh(np.concatenate([pa, pb]), np.concatenate([ta, tb + len(pa)])), "strip10245")
    assert got["shell_counts"][:, 0].tolist() == [40 * 256 + 5, 7]


# ---- 3. seams: an unwelded mesh's shells are the welded mesh's
def scene_mesh(which):
    if which == "smooth":
        with open(os.path.join(GOLD, "obj", "smooth.obj"), "rb") as f:
            return hc.Mesh.from_obj(f.read(), os.path.join(GOLD, "obj"))
    return hc.Mesh.from_obj(og.scene(mg.torus(24, 26, polys="mixed"), normals="smooth", tex="atlas", charts=5).obj, "")


@pytest.mark.parametrize("which", ["smooth", "atlas"])
def test_seams(cx, which):
    mesh = scene_mesh(which)
    got, _ = check(cx, mesh, which)
    split = cx.shells_stat()
    rn = cx.render_numpy(mesh)
    vs = rn["vertex_source"]
    assert len(vs) > mesh.nv                                       # the render build has split vertices
    P = np.zeros((mesh.nv, 3), np.float32)
    P[vs] = rn[f"list{position_list(mesh)}"][:, :3]
    deg = np.diff(mesh.face_offsets().astype(np.int64))
    v = np.zeros(mesh.nv, np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4")]))
    v["x"], v["y"], v["z"] = P[:, 0], P[:, 1], P[:, 2]
    w = cx.shells_numpy(hc.Mesh.from_arrays(v, deg.astype(np.uint8), mesh.org()))
    assert np.array_equal(got["tri_shell"], w["tri_shell"]) and np.array_equal(got["shell_counts"], w["shell_counts"])
    assert all(cx.shells_stat()[k] == split[k] for k in SUMMARY)


# ---- 4. decoded meshes: resident or not, the same bytes
@pytest.mark.parametrize("profile", [hc.PROFILE_COMPAT, hc.PROFILE_CHUNKED], ids=["compat", "chunked"])
@pytest.mark.parametrize("bits", [0, 12], ids=["lossless", "q12"])
def test_decoded(cx, profile, bits):
    m = mesh_of(mg.torus(24, 16, polys="mixed"))
    if bits:
        cx.requant(m, [(1, -1, bits)])
    dec = cx.read_hry(cx.write_hry(m, profile=profile))
    first = cx.shells_numpy(dec, geometry=True)         # straight after the decode
    cx.bounds(mesh_of(mg.grid(4, 4)))                   # another call touches the context
    again = cx.shells_numpy(dec, geometry=True)
    same_bytes(first, again)
    compare(first, restated(cx, dec), f"decoded profile {profile} bits {bits}")


# ---- 5. determinism
def test_two_builds_same_bytes(cx):
    for mesh in (mesh_of(mg.soup()), mesh_of(mg.torus(40, 30, polys="mixed")), mesh_of(mg.multi_component(3, 8, 6))):
        same_bytes(cx.shells_numpy(mesh, geometry=True), cx.shells_numpy(mesh, geometry=True))


# ---- 6. degenerate triangles (integer-lattice coordinates: every product and sum is exact)
def test_degenerate(cx):
    pos = [[0, 0, 0], [2, 0, 0], [0, 2, 0], [4, 0, 0], [np.nan, -0.0, 1], [1, 1, -3]]
    # good, a repeated index, three collinear corners, a NaN corner, good
    tris = [[0, 1, 2], [0, 1, 1], [0, 1, 3], [1, 0, 4], [0, 1, 5]]
    got, _ = check(cx, xyz_mesh(pos, tris), "degenerate")
    m = got["shell_measures"]
    assert len(m) == 1 and not np.isnan(m).any()
    # triangle 0 adds 4, triangle 4 adds |(2, 0, 0) x (1, 1, -3)| = |(0, 6, 2)| = sqrt(40); the others exactly +0
    assert er.float_steps(m[0, :1], np.array([0.5 * (4.0 + np.sqrt(np.float64(40.0)))], np.float32))[1] <= 1
    assert m[0, 1] == 0.0 and not np.signbit(m[0, 1])           # every volume term has a = P0 - O = 0 or is not finite
    assert m[0, 2:].tolist() == [0, 0, -3, 4, 2, 1] and np.signbit(m[0, 3])   # the box skips the NaN and puts -0 below +0
    got, _ = check(cx, xyz_mesh([[np.nan] * 3] * 3, [[0, 1, 2]]), "all-NaN")
    assert got["shell_measures"][0].tolist() == [0, 0, np.inf, np.inf, np.inf, -np.inf, -np.inf, -np.inf]


def test_no_triangles(cx):
    v = np.zeros(3, np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4")]))
    got = cx.shells_numpy(hc.Mesh.from_arrays(v, np.zeros(0, np.uint8), np.zeros(0, np.uint32)), geometry=True)
    assert sorted(got) == sorted(sr.FIXED + sr.GEOMETRY) and all(a.shape[0] == 0 for a in got.values())   # isolated vertices belong to no shell
    assert got["shell_counts"].shape == (0, 8) and got["shell_measures"].shape == (0, 8)
    assert tuple(cx.shells_stat()[k] for k in SUMMARY) == (0, 0, 0, 0, 0, 0)


# ---- 7. refusals
def raw_build(cx, mesh, render_of, edges_of, flags):
    """hry_shells_build of `mesh` with a render build of `render_of` and an edges build of `edges_of`: (status, handle value, error text)"""
    L = nat.load()
    r, r2, e, s = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(1)
    nat.check(L.hry_render_build(cx.h, render_of.h, C.byref(r)))
    nat.check(L.hry_render_build(cx.h, edges_of.h, C.byref(r2)))
    try:
        nat.check(L.hry_edges_build(cx.h, edges_of.h, r2, 0, C.byref(e)))
        try:
            rc = L.hry_shells_build(cx.h, mesh.h, r, e, flags, C.byref(s))
            text = L.hry_last_error() if rc else b""
            if rc == 0:
                L.hry_shells_free(s)
            return rc, (s.value if rc else None), text
        finally:
            L.hry_edges_free(e)
    finally:
        L.hry_render_free(r)
        L.hry_render_free(r2)


def test_refusals(cx):
    good = xyz_mesh([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 1, 2]])
    other = mesh_of(mg.torus(12, 10))
    flat = np.zeros(3, np.dtype([("x", "<f4"), ("y", "<f4")]))
    flat["x"], flat["y"] = [0, 1, 0], [0, 0, 1]
    xy = hc.Mesh.from_arrays(flat, np.array([3], np.uint8), np.array([0, 1, 2], np.uint32))

    def usable():
        assert raw_build(cx, good, good, good, 1)[0] == 0
        check(cx, good)

    for flags in (2, 1 | 4, 0x80000000):
        rc, h, text = raw_build(cx, good, good, good, flags)
        assert rc == nat.E_ARG and not h and text
        usable()
    rc, h, text = raw_build(cx, good, other, good, 0)      # a render of another mesh
    assert rc == nat.E_ARG and not h and b"render" in text
    usable()
    rc, h, text = raw_build(cx, good, good, other, 0)      # edges of another mesh
    assert rc == nat.E_ARG and not h and b"edge" in text
    usable()
    rc, h, text = raw_build(cx, xy, xy, xy, 1)             # geometry without a z
    assert rc == nat.E_UNSUPPORTED and not h and b"position" in text
    usable()
    assert raw_build(cx, xy, xy, xy, 0)[0] == 0            # ... the topology alone builds
    got, want = check(cx, xy, geometry=False)
    assert got["shell_counts"].tolist() == [[1, 1, 3, 3, 3, 0, 0, 1]]
    with pytest.raises(hc.HryError):
        cx.shells_numpy(xy, geometry=True)
    usable()
    L = nat.load()
    r, e = C.c_void_p(), C.c_void_p()
    nat.check(L.hry_render_build(cx.h, good.h, C.byref(r)))
    nat.check(L.hry_edges_build(cx.h, good.h, r, 0, C.byref(e)))
    for args in ((None, good.h, r, e), (cx.h, None, r, e), (cx.h, good.h, None, e), (cx.h, good.h, r, None)):
        s = C.c_void_p(1)
        assert L.hry_shells_build(*args, 0, C.byref(s)) == nat.E_ARG and not s.value
    assert L.hry_shells_build(cx.h, good.h, r, e, 0, None) == nat.E_ARG
    L.hry_edges_free(e)
    L.hry_render_free(r)
    usable()


def test_handle_outlives_inputs_and_get(cx):
    """the handle owns its memory (render and edges are freed before any buffer is read), and hry_shells_get describes the buffers"""
    mesh = mesh_of(mg.multi_component(3, 8, 6))
    L = nat.load()
    r, e, s = C.c_void_p(), C.c_void_p(), C.c_void_p()
    nat.check(L.hry_render_build(cx.h, mesh.h, C.byref(r)))
    nat.check(L.hry_edges_build(cx.h, mesh.h, r, 0, C.byref(e)))
    nat.check(L.hry_shells_build(cx.h, mesh.h, r, e, 1, C.byref(s)))
    E = L.hry_edges_count(e)
    L.hry_edges_free(e)
    L.hry_render_free(r)
    try:
        S, T = L.hry_shells_count(s), mesh.ntri
        assert S == 3
        shapes = {"tri_shell": (T, 1, 4), "face_shell": (mesh.nf, 1, 4), "edge_shell": (E, 1, 4), "shell_first": (S, 1, 4), "shell_counts": (S, 8, 4),
                  "shell_measures": (S, 8, 0), "no_such": (0, 0, 0)}
        for name, want in shapes.items():
            dev, rows, width, typ = C.c_void_p(), C.c_uint64(), C.c_int(), C.c_int()
            nat.check(L.hry_shells_get(s, name.encode(), C.byref(dev), C.byref(rows), C.byref(width), C.byref(typ)))
            assert (rows.value, width.value, typ.value) == want and bool(dev.value) == (name != "no_such"), name
        first = np.empty(S, np.uint32)
        nat.check(L.hry_shells_copy(cx.h, s, b"shell_first", first.ctypes.data, 0))
        assert np.array_equal(first, np.arange(3) * (T // 3))
        assert L.hry_shells_copy(cx.h, s, b"no_such", first.ctypes.data, 0) == nat.E_ARG
        t = (C.c_uint64 * 6)()
        nat.check(L.hry_shells_summary(s, t))
        assert list(t) == [3, 3, 0, 0, 0, T // 3]
        d, up = C.c_double(), C.c_uint64(7)
        nat.check(L.hry_shells_stat(s, C.byref(d), C.byref(up)))
        assert d.value > 0 and up.value == 0
    finally:
        L.hry_shells_free(s)


# ---- 8. the command line
def run_cli(*args):
    r = subprocess.run([cli.HARRY] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def shells_lines(out):
    head = [l.split() for l in out.splitlines() if l.startswith("Shells:")]
    rows = [l.split() for l in out.splitlines() if l.startswith("Shell:")]
    assert len(head) == 1 and head[0][1::2] == ["shells", "closed", "nonmanifold", "misoriented", "loops", "largest"], out
    for w in rows:
        assert w[2::2] == ["triangles", "vertices", "edges", "boundary", "loops", "euler", "genus"], w
    return dict(zip(head[0][1::2], map(int, head[0][2::2]))), [[w[1]] + w[3::2] for w in rows]


def test_shells_option(cx, tmp_path):
    (tmp_path / "multi.ply").write_bytes(mg.multi_component(3, 8, 6, polys="tri").to_ply())
    (tmp_path / "soup.ply").write_bytes(mg.soup().to_ply())
    (tmp_path / "ico.ply").write_bytes(mg.icosphere(2).to_ply())
    out = run_cli(tmp_path / "multi.ply", "--shells")
    head, rows = shells_lines(out)
    assert head == {"shells": 3, "closed": 3, "nonmanifold": 0, "misoriented": 0, "loops": 0, "largest": 96} and "Writing output" not in out
    assert rows == [[str(i), "96", "48", "144", "0", "0", "0", "1"] for i in range(3)]
    head, rows = shells_lines(run_cli(tmp_path / "soup.ply", "--shells"))
    want = restated(cx, mesh_of(mg.soup()), geometry=False)
    assert tuple(head.values()) == want["summary"] and len(rows) == 16       # the first 16 of 39 shells
    for i, w in enumerate(rows):
        c = want["shell_counts"][i]
        g = sr.genus(c)
        assert w == [str(i), str(c[0]), str(c[2]), str(c[3]), str(c[4]), str(c[7]), str(sr.euler(c)), "-" if g is None else str(g)]
    assert any(w[-1] == "-" for w in rows)
    plain = subprocess.run([cli.HARRY, str(tmp_path / "ico.ply"), str(tmp_path / "plain.hry")], capture_output=True, text=True, timeout=300)
    out = run_cli(tmp_path / "ico.ply", tmp_path / "ico.hry", "--shells")
    head, rows = shells_lines(out)
    assert head["shells"] == 1 and head["closed"] == 1 and rows[0][-2:] == ["2", "0"]
    assert (tmp_path / "ico.hry").read_bytes() == (tmp_path / "plain.hry").read_bytes()
    keep = lambda text: [l for l in text.splitlines() if not l.startswith(("Shells:", "Shell:", "Topology:")) and " took " not in l and "time" not in l]
    assert keep(out) == keep(plain.stdout)                  # the other output is unchanged
    head, rows = shells_lines(run_cli(tmp_path / "ico.hry", "--shells"))   # a .hry input: the decoded mesh
    assert head["shells"] == 1 and rows[0][-2:] == ["2", "0"]
    alone = run_cli(tmp_path / "ico.ply", "--topology")
    both = run_cli(tmp_path / "ico.ply", "--topology", "--shells")
    marked = [l for l in both.splitlines() if l.startswith(("Topology:", "Shells:", "Shell:"))]
    assert [l.split(":")[0] for l in marked] == ["Topology", "Shells", "Shell"]
    assert marked[0] == [l for l in alone.splitlines() if l.startswith("Topology:")][0]
    r = subprocess.run([cli.HARRY, str(tmp_path / "ico.ply")], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "Too few non-optional arguments" in r.stderr    # without either option the output stays mandatory


# ---- 9. torch: Codec.shells
TORCH_CHILD = r"""
import sys
import numpy as np
import torch
torch.cuda.init()   # a PyTorch program: torch holds the device before the codec starts
sys.path.insert(0, sys.argv[1])
from harry_amd import codec as hc
from harry_amd import meshgen as mg
m = mg.multi_component(3, 8, 6)
mesh = hc.Mesh.from_arrays(m.verts, m.degrees, m.indices)
c = hc.Codec(0)
ref = c.shells_numpy(mesh, geometry=True)
got = c.shells(mesh, geometry=True)
assert sorted(got) == sorted(ref)
for k, t in got.items():
    assert t.device == torch.device("cuda", 0) and t.dtype == (torch.float32 if ref[k].dtype == np.float32 else torch.int32), k
    assert tuple(t.shape) == ref[k].shape and np.array_equal(t.cpu().numpy().view(np.uint8), ref[k].view(np.uint8)), k
assert sorted(c.shells(mesh)) == sorted(c.shells_numpy(mesh)) and "shell_measures" not in c.shells(mesh)
st = c.shells_stat()
assert st["shells"] == 3 and st["closed"] == 3 and st["uploaded_bytes"] == 0 and st["largest"] == mesh.ntri // 3
tri = torch.nonzero(got["tri_shell"] == 1).flatten()   # "the triangles of component k" without a label-propagation loop
assert tri.numel() == mesh.ntri // 3
c.close()
print("torch ok")
"""


def test_torch_tensors():
    pytest.importorskip("torch")
    r = subprocess.run([sys.executable, "-c", TORCH_CHILD, util.ROOT], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "torch ok" in r.stdout, r.stdout + r.stderr
