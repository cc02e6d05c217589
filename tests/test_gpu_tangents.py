"""Tangent frames of a render build (include/harry_amd.h: hry_tangents_build; kernels: harry_amd/csrc/device/tangents.hip) against
the numpy restatement of tests/tangents_ref.py, which reads what the render build holds per output vertex.  Tangent and bitangent
components are compared within tangents_ref.TOL on the vertices its guard admits -- every test asserts that it admits all --, the
handedness w, the zero rows and the summary's counts exactly."""
import ctypes as C
import subprocess
import sys

import numpy as np
import pytest

from harry_amd import _native as nat
from harry_amd import cli
from harry_amd import codec as hc
from harry_amd import meshgen as mg
from tests import tangents_ref as tr
from tests import util

pytestmark = pytest.mark.gpu

WEIGHTS = ("area", "angle")
SUMMARY = ("framed", "unframed", "mirrored", "mixed", "degenerate")


@pytest.fixture(scope="module")
def cx():
    c = hc.Codec(0)
    yield c
    c.close()


# ---- meshes with texture coordinates
def planar(x, y, flip_u=False):
    u, v = 0.8 * x + 0.6 * y, -0.6 * x + 0.8 * y
    return (-u if flip_u else u), v


def with_uv(m, uv=None, flip_u=False):
    """a PLY-layout mesh x y z u v from a meshgen mesh; uv: [nv, 2], default the planar map"""
    x, y, z = (np.asarray(m.verts[k], np.float32) for k in "xyz")
    u, v = planar(x, y, flip_u) if uv is None else np.asarray(uv, np.float32).T
    verts = np.zeros(len(x), np.dtype([(k, "<f4") for k in ("x", "y", "z", "u", "v")]))
    verts["x"], verts["y"], verts["z"], verts["u"], verts["v"] = x, y, z, u, v
    return hc.Mesh.from_arrays(verts, m.degrees, m.indices)


def arrays_mesh(pos, uv, tris):
    pos, tris = np.asarray(pos, np.float32), np.asarray(tris, np.uint32).reshape(-1, 3)
    verts = util.xyz(pos)
    return with_uv(mg.Mesh(verts, np.full(len(tris), 3, np.uint8), tris.reshape(-1)), uv)


def torus_obj(nu=24, nv=16, flip_u=False, normals=False, no_vt_faces=0):
    """the triangles of mg.torus(nu, nv) as OBJ text with a parametric uv per corner: (minor angle, major angle) / 2 pi, unwrapped
    per cell, so that a face across the wrap names vt records one period up and the seam's vertices get two of them.  normals: vn
    lines, the analytic outward normal per vertex.  no_vt_faces: the last so many faces are written without vt"""
    m = mg.torus(nu, nv)
    # (fixed notation throughout: the reader ignores the sign of an exponent, as the reference's does)
    lines = ["v %.10f %.10f %.10f" % (float(p["x"]), float(p["y"]), float(p["z"])) for p in m.verts]
    for iu in range(nu + 1):
        for iv in range(nv + 1):
            u = iv / nv
            lines.append("vt %.10f %.10f" % (-u if flip_u else u, iu / nu))
    if normals:
        for iu in range(nu):
            for iv in range(nv):
                a, b = 2 * np.pi * iu / nu, 2 * np.pi * iv / nv
                lines.append("vn %.10f %.10f %.10f" % (np.cos(b) * np.cos(a), np.cos(b) * np.sin(a), np.sin(b)))
    faces = []
    for iu in range(nu):
        for iv in range(nv):
            cell = {"a": (iu, iv), "b": (iu, iv + 1), "c": (iu + 1, iv + 1), "d": (iu + 1, iv)}
            faces += [[cell[k] for k in "abc"], [cell[k] for k in "acd"]]
    for f, corners in enumerate(faces):
        words = []
        for ju, jv in corners:
            vtx = (ju % nu) * nv + jv % nv + 1
            vt = ju * (nv + 1) + jv + 1
            if f >= len(faces) - no_vt_faces:
                words.append("%d//%d" % (vtx, vtx) if normals else "%d" % vtx)
            else:
                words.append("%d/%d/%d" % (vtx, vt, vtx) if normals else "%d/%d/" % (vtx, vt))   # ("v/t" would name normal t as well)
        lines.append("f " + " ".join(words))
    return ("\n".join(lines) + "\n").encode()


def lists_with(mesh, interp, ncomp):
    L = nat.load()
    return [l for l in range(mesh.nlists) if mesh.list_target(l) in (1, 2) and L.hry_list_interp_ncomp(mesh.h, l, interp) >= ncomp]


def inputs(cx, mesh, normals="area"):
    """what the contract reads of the mesh's render build: positions, uv, normals per output vertex, and the triangles"""
    rn = cx.render_numpy(mesh, normals=None if normals == "stored" else normals)
    (pl,), (tl,) = lists_with(mesh, 0, 3), lists_with(mesh, 16, 2)
    at = 3 if tl == pl else 0   # (the test meshes' vertex records are x y z u v; OBJ lists start with their own components)
    nrm = rn[f"list{lists_with(mesh, 1, 3)[0]}"][:, :3] if normals == "stored" else rn["normals"]
    return rn[f"list{pl}"][:, :3], rn[f"list{tl}"][:, at:at + 2], nrm, rn["indices"], rn


def not_bit_equal(a, b):
    return int((np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)).sum())


def compare(got, want, label):
    g, w = got["tangents"], want["tangents"]
    assert g.dtype == np.float32 and g.shape == w.shape
    assert want["guard"].all(), (label, "the guard excludes", int((~want["guard"]).sum()))
    zero = ~w.any(axis=1)
    assert np.array_equal(~g.any(axis=1), zero) and not g[zero].view(np.uint32).any(), label
    assert np.array_equal(g[:, 3], w[:, 3]), (label, "w differs at", np.nonzero(g[:, 3] != w[:, 3])[0][:8])
    err = float(np.abs(g[:, :3].astype(np.float64) - w[:, :3]).max()) if len(g) else 0.0
    print(label, "tangents: values not bit-equal:", not_bit_equal(g, w), "of", g.size, "largest difference:", err)
    assert err <= tr.TOL, (label, err)
    if "bitangents" in got:
        b, wb = got["bitangents"], want["bitangents"]
        assert b.dtype == np.float32 and b.shape == wb.shape and not b[zero].view(np.uint32).any()
        err = float(np.abs(b.astype(np.float64) - wb).max()) if len(b) else 0.0
        print(label, "bitangents: values not bit-equal:", not_bit_equal(b, wb), "of", b.size, "largest difference:", err)
        assert err <= tr.TOL, (label, err)


def check(cx, mesh, label, normals="area"):
    """every combination of weights and bitangents against the restatement, with the summary and the stat; returns the restatement
    and the buffers per weights (with bitangents)"""
    pos, uv, nrm, idx, rn = inputs(cx, mesh, normals)
    out = {}
    for weights in WEIGHTS:
        want = tr.tangents(pos, uv, nrm, idx, weights)
        for bit in (False, True):
            got = cx.tangents_numpy(mesh, normals=normals, weights=weights, bitangents=bit)
            st = cx.tangents_stat()
            assert sorted(got) == sorted(["tangents", "indices", "vertex_source"] + (["bitangents"] if bit else []))
            assert np.array_equal(got["indices"], rn["indices"]) and np.array_equal(got["vertex_source"], rn["vertex_source"])
            assert st["uploaded_bytes"] == 0 and st["device_ms"] > 0
            assert tuple(st[k] for k in SUMMARY) == want["summary"], (label, weights, st, want["summary"])
            compare(got, want, f"{label} {weights}")
        out[weights] = (want, got)
    return out


# ---- 1. against the restatement
def test_grid(cx):
    for quads in (False, True):
        r = check(cx, with_uv(mg.grid(9, 8, quads=quads)), f"grid quads={quads}")
        # (the grid's faces are wound clockwise seen from +z: the normals point down and the planar map is mirrored throughout)
        assert r["area"][0]["summary"] == (72, 0, 72, 0, 0)


@pytest.mark.parametrize("name", ["icosphere", "torus"])
def test_planar_map_on_closed_surfaces(cx, name):
    m = mg.icosphere(2) if name == "icosphere" else mg.torus(24, 16)
    r = check(cx, with_uv(m), name)
    for weights in WEIGHTS:   # the far side of a planar map is mirrored, and the silhouette mixes both signs
        s = r[weights][0]["summary"]
        assert s[2] > 0 and s[3] > 0, (weights, s)


def test_obj_torus_unwelded(cx):
    mesh = hc.Mesh.from_obj(torus_obj(), "")
    r = check(cx, mesh, "obj torus")
    want, got = r["area"]
    U = len(got["tangents"])
    assert U > mesh.nv and want["summary"] == (U, 0, 0, 0, 0) and (got["tangents"][:, 3] == 1).all()
    flipped = check(cx, hc.Mesh.from_obj(torus_obj(flip_u=True), ""), "obj torus -u")["area"]
    assert flipped[0]["summary"] == (U, 0, U, 0, 0) and (flipped[1]["tangents"][:, 3] == -1).all()
    assert np.array_equal(flipped[1]["tangents"][:, :3], -got["tangents"][:, :3])


def test_obj_torus_stored_normals(cx):
    mesh = hc.Mesh.from_obj(torus_obj(normals=True), "")
    r = check(cx, mesh, "obj torus vn", normals="stored")
    want, got = r["area"]
    assert want["summary"][0] == len(got["tangents"]) > mesh.nv and want["summary"][3] == 0
    assert len(set(got["tangents"][:, 3].tolist())) == 1   # one handedness: the normals all point the same way relative to the winding


# ---- 2. the seams of the kernels
def strip(ntri):
    """the first ntri triangles of a two-row grid"""
    m = mg.grid(ntri // 2 + 2, 2)
    tris = m.indices.reshape(-1, 3)[:ntri]
    assert len(tris) == ntri
    return mg.Mesh(m.verts, np.full(ntri, 3, np.uint8), tris.reshape(-1))


SEAMS = {
    "hubs_32_33": lambda: mg.hub_discs([32, 33]),       # the last lane-summed segment and the first hub
    "hubs_64_65": lambda: mg.hub_discs([64, 65]),
    "hubs_257_300": lambda: mg.hub_discs([257, 300]),   # lengths that are no multiple of 256: the ranges are uneven
    "vertices_64": lambda: mg.grid(8, 8),               # U either side of a wavefront
    "vertices_65": lambda: mg.grid(13, 5),
    "strip21": lambda: strip(21),                       # 3 T = 63, 66: either side of a wavefront of slots
    "strip22": lambda: strip(22),
    "strip257": lambda: strip(257),                     # more triangles than one block of the triangle kernel
}


@pytest.mark.parametrize("name", sorted(SEAMS))
def test_seams(cx, name):
    m = SEAMS[name]()
    r = check(cx, with_uv(m), name)
    if name.startswith("hubs"):
        valences = np.bincount(m.indices, minlength=m.nv)
        want = [int(x) for x in name.split("_")[1:]]
        assert sorted(valences[valences >= 32].tolist()) == want
    if name.startswith("vertices"):
        assert m.nv == int(name.split("_")[1])
    assert r["area"][0]["summary"][:2] == (len(np.unique(m.indices)), m.nv - len(np.unique(m.indices)))   # (a strip leaves grid vertices unused)


# ---- 3. designed zeros, and the mixed vertex
def test_designed_zeros(cx):
    pos = [[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.1],      # a proper pair of triangles
           [3, 0, 0], [4, 0, 0], [3, 1, 0],                    # one uv at all corners
           [6, 0, 0], [7, 0, 0], [6, 1, 0],                    # a NaN uv
           [9, 9, 9]]                                          # isolated
    uv = [[0, 0], [1, 0], [0, 1], [1, 1], [0.5, 0.5], [0.5, 0.5], [0.5, 0.5], [0, 0], [np.nan, 0], [0, 1], [0.25, 0.25]]
    mesh = arrays_mesh(pos, uv, [[0, 1, 2], [1, 3, 2], [4, 5, 6], [7, 8, 9]])
    for weights in WEIGHTS:
        want, got = check(cx, mesh, "zeros")[weights]
        assert want["summary"] == (4, 7, 0, 0, 2)
        assert got["tangents"][:4].any(axis=1).all() and not got["tangents"][4:].view(np.uint32).any() and not got["bitangents"][4:].view(np.uint32).any()


def test_obj_faces_without_vt(cx):
    mesh = hc.Mesh.from_obj(torus_obj(6, 5, no_vt_faces=7), "")
    for weights in WEIGHTS:
        want, got = check(cx, mesh, "obj no vt")[weights]
        assert want["summary"][4] == 7 and want["summary"][1] > 0
        assert np.array_equal(~got["tangents"].any(axis=1), ~want["tangents"].any(axis=1))


def test_butterfly_is_mixed(cx):
    pos = [[0, 0, 0], [1, 0, 0], [0, 1, 0], [-1, 0, 0], [-1, -1, 0]]
    # the second wing's uv are wound against its positions; its shape and stretch keep the two bitangent terms from cancelling
    uv = [[0, 0], [1, 0], [0, 1], [-2, 0], [0, 1]]
    mesh = arrays_mesh(pos, uv, [[0, 1, 2], [0, 3, 4]])
    want, got = check(cx, mesh, "butterfly")["area"]
    assert want["summary"][3] == 1 and want["mixed"].tolist() == [True, False, False, False, False]


# ---- 4. determinism
def same_bits(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


def test_three_builds_are_bit_identical(cx):
    mesh = with_uv(mg.hub_discs([40, 300]))
    for weights in WEIGHTS:
        first = cx.tangents_numpy(mesh, weights=weights, bitangents=True)
        for _ in range(2):
            same_bits(cx.tangents_numpy(mesh, weights=weights, bitangents=True), first)


@pytest.mark.parametrize("profile", [hc.PROFILE_COMPAT, hc.PROFILE_CHUNKED], ids=["compat", "chunked"])
@pytest.mark.parametrize("bits", [0, 12], ids=["lossless", "q12"])
def test_resident_and_uploaded(cx, profile, bits):
    m = with_uv(mg.torus(24, 16))
    if bits:
        cx.requant(m, [(1, -1, bits)])
    dec = cx.read_hry(cx.write_hry(m, profile=profile))
    resident = cx.tangents_numpy(dec, bitangents=True)   # (a render build leaves the decode's buffers where they are)
    assert cx.tangents_stat()["render_uploaded_bytes"] == 0 and cx.tangents_stat()["uploaded_bytes"] == 0
    compare(resident, tr.tangents(*inputs(cx, dec)[:4]), f"resident {bits}")
    up = dec.clone()
    same_bits(cx.tangents_numpy(up, bitangents=True), resident)
    assert cx.tangents_stat()["render_uploaded_bytes"] > 0 and cx.tangents_stat()["uploaded_bytes"] == 0


TORCH_CHILD = r"""
import sys
import numpy as np
import torch
torch.cuda.init()   # a PyTorch program: torch holds the device before the codec starts
sys.path.insert(0, sys.argv[1])
from harry_amd import codec as hc
from harry_amd import meshgen as mg
from tests.test_gpu_tangents import with_uv
mesh = with_uv(mg.hub_discs([33, 64]))
c = hc.Codec(0)
for weights in ("area", "angle"):
    ref = c.tangents_numpy(mesh, normals="angle", weights=weights, bitangents=True)
    got = c.tangents(mesh, normals="angle", weights=weights, bitangents=True)
    assert sorted(got) == sorted(ref) == ["bitangents", "indices", "tangents", "vertex_source"]
    for k, t in got.items():
        assert t.device == torch.device("cuda", 0) and t.dtype == (torch.float32 if ref[k].dtype == np.float32 else torch.int32), k
        assert tuple(t.shape) == ref[k].shape and np.array_equal(t.cpu().numpy().view(np.uint8), ref[k].view(np.uint8)), k
assert "bitangents" not in c.tangents(mesh)
st = c.tangents_stat()
assert st["framed"] == mesh.nv and st["uploaded_bytes"] == 0
c.close()
print("torch ok")
"""


def test_torch_tensors():
    pytest.importorskip("torch")
    r = subprocess.run([sys.executable, "-c", TORCH_CHILD, util.ROOT], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "torch ok" in r.stdout, r.stdout + r.stderr


# ---- 5. refusals: *out stays NULL and a good build follows
def test_refusals(cx):
    L = nat.load()
    good = with_uv(mg.grid(4, 4))
    no_uv = util.xyz_mesh([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 1, 2]])
    with_vn = hc.Mesh.from_obj(torus_obj(6, 5, normals=True), "")

    def render(mesh, flags):
        r = C.c_void_p()
        nat.check(L.hry_render_build_ex(cx.h, mesh.h, flags, C.byref(r)))
        return r

    def refused(mesh, r, flags, code, *words):
        out = C.c_void_p(1)
        assert L.hry_tangents_build(cx.h, mesh.h, r, flags, C.byref(out)) == code and not out.value
        text = L.hry_last_error().decode()
        assert all(w in text for w in words), text
        frames = cx.tangents_numpy(good)
        assert frames["tangents"].any(axis=1).all()

    VN = hc.Codec.RENDER_VERTEX_NORMALS
    handles = [render(no_uv, VN), render(good, 0), render(good, VN), render(with_vn, VN)]
    try:
        refused(no_uv, handles[0], 0, nat.E_UNSUPPORTED, "no vertex or corner list", "texture-coordinate")
        refused(good, handles[1], 0, nat.E_ARG, "HRY_RENDER_VERTEX_NORMALS")
        refused(good, handles[2], nat.TANGENTS_STORED_NORMALS, nat.E_UNSUPPORTED, "no vertex or corner list", "normal")
        refused(good, handles[2], 8, nat.E_ARG, "unknown tangents flag")
        refused(good, handles[3], 0, nat.E_ARG, "not a render build of this mesh")
        refused(with_vn, handles[2], 0, nat.E_ARG, "not a render build of this mesh")
        out = C.c_void_p(1)
        assert L.hry_tangents_build(cx.h, good.h, None, 0, C.byref(out)) == nat.E_ARG and not out.value
        t = C.c_void_p()
        nat.check(L.hry_tangents_build(cx.h, with_vn.h, handles[3], nat.TANGENTS_STORED_NORMALS | nat.TANGENTS_BITANGENTS, C.byref(t)))
        rows = C.c_uint64()
        nat.check(L.hry_tangents_get(t, b"bitangents", None, C.byref(rows), None, None))
        assert rows.value == L.hry_render_nverts(handles[3]) == L.hry_tangents_count(t)
        L.hry_tangents_free(t)
    finally:
        for r in handles:
            L.hry_render_free(r)


# ---- 6. the command line
def test_tangents_option(cx, tmp_path):
    (tmp_path / "scene.obj").write_bytes(torus_obj())
    mesh = hc.Mesh.from_obj(torus_obj(), "")
    want = tr.tangents(*inputs(cx, mesh)[:4])
    r = subprocess.run([cli.HARRY, str(tmp_path / "scene.obj"), "--tangents"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l.split() for l in r.stdout.splitlines() if l.startswith("Tangents:")]
    assert len(lines) == 1 and tuple(lines[0][1::2]) == ("vertices",) + SUMMARY and "Writing output" not in r.stdout
    assert tuple(map(int, lines[0][2::2])) == (len(want["tangents"]),) + want["summary"]
    (tmp_path / "plain.ply").write_bytes(mg.torus(6, 5).to_ply())
    r = subprocess.run([cli.HARRY, str(tmp_path / "plain.ply"), "--tangents"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "texture-coordinate" in r.stderr and "Tangents:" not in r.stdout
