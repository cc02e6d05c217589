"""Normals of a render build (include/harry_amd.h: hry_render_build_ex; kernels: harry_amd/csrc/device/normals.hip) against the numpy
float64 restatement of tests/normals_ref.py, at its derived tolerance of 2^-24 per component on vertices whose sum does not cancel
(every test asserts that the guard excluded none), and exact zeros on the designed degenerate cases."""
import ctypes as C
import os

import numpy as np
import pytest

from harry_amd import _native as nat
from harry_amd import codec as hc
from harry_amd import meshgen as mg
from harry_amd import objgen as og
from tests import normals_ref as nr
from tests import util

pytestmark = pytest.mark.gpu

GOLD = os.path.join(util.ROOT, "tests", "golden")
MODES = ("area", "angle")
VN, FN, ANGLE = 1, 2, 4


@pytest.fixture(scope="module")
def cx():
    c = hc.Codec(0)
    yield c
    c.close()


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def mesh_of(m):
    return hc.Mesh.from_arrays(m.verts, m.degrees, m.indices)


def xyz_mesh(pos, degrees, indices):
    pos = np.asarray(pos, np.float32)
    v = np.zeros(len(pos), np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4")]))
    v["x"], v["y"], v["z"] = pos[:, 0], pos[:, 1], pos[:, 2]
    return hc.Mesh.from_arrays(v, np.asarray(degrees, np.uint8), np.asarray(indices, np.uint32))


def position_list(mesh):
    ls = [l for l in range(mesh.nlists) if mesh.list_target(l) == 1 and len(mesh.list_fmt(l)) >= 3]
    assert len(ls) == 1
    return ls[0]


def positions(mesh, got):
    """float32 [nv, 3]: what the build's list buffer holds for every decoded vertex"""
    rows = got[f"list{position_list(mesh)}"][:, :3]
    P = np.zeros((mesh.nv, 3), np.float32)
    P[got["vertex_source"]] = rows
    return P


def restated(mesh, got, mode):
    return nr.normals(positions(mesh, got), np.diff(mesh.face_offsets().astype(np.int64)), mesh.org(), mode)


def close(got, want, rows=None):
    assert got.dtype == np.float32 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    d = np.abs(got.astype(np.float64) - want.astype(np.float64))
    if rows is not None:
        d = d[rows]
    worst = float(d.max()) if d.size else 0.0
    print("largest difference", worst, "of", nr.TOL)
    assert np.isfinite(got).all() and worst <= nr.TOL, worst


def check(cx, mesh, modes=MODES):
    """both modes and the face normals against the restatement; returns the buffers per mode"""
    out = {}
    for mode in modes:
        got = cx.render_numpy(mesh, normals=mode, face_normals=True)
        fn, vn, guard = restated(mesh, got, mode)
        assert int((~guard).sum()) == 0   # the guard hides nothing
        assert got["face_normals"].shape == (mesh.nf, 3) and got["normals"].shape == (len(got["vertex_source"]), 3)
        close(got["face_normals"], fn)
        close(got["normals"], vn[got["vertex_source"]], guard[got["vertex_source"]])
        out[mode] = got
    return out


def same_bits(a, b, keys=("normals", "face_normals")):
    for k in keys:
        assert a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


# ---- 1. both modes and face normals
MESHES = {
    "torus_tri": lambda: mg.torus(24, 16),
    "torus_mixed": lambda: mg.torus(24, 16, polys="mixed"),
    "torus_far": lambda: mg.torus(24, 16, center=(1e4, -2e4, 3e4)),
    "grid_quads": lambda: mg.grid(9, 8, quads=True),
    "icosphere": lambda: mg.icosphere(2),
    "nonmanifold": lambda: mg.with_nonmanifold(mg.torus(12, 10)),
    "soup": lambda: mg.soup(),
}


@pytest.mark.parametrize("name", sorted(MESHES))
def test_against_restatement(cx, name):
    check(cx, mesh_of(MESHES[name]()))


# ---- 2. lossless and quantised, resident and uploaded
@pytest.mark.parametrize("profile", [hc.PROFILE_COMPAT, hc.PROFILE_CHUNKED], ids=["compat", "chunked"])
@pytest.mark.parametrize("bits", [0, 12], ids=["lossless", "q12"])
def test_resident_and_uploaded(cx, profile, bits):
    m = mesh_of(mg.torus(24, 16, polys="mixed"))
    if bits:
        cx.requant(m, [(1, -1, bits)])
    dec = cx.read_hry(cx.write_hry(m, profile=profile))
    resident = {}
    for mode in MODES:   # (a render leaves the decode's buffers where they are: both builds are resident)
        resident[mode] = check(cx, dec, (mode,))[mode]
        assert cx.render_stat()["uploaded_bytes"] == 0
    up = dec.clone()
    for mode in MODES:
        got = cx.render_numpy(up, normals=mode, face_normals=True)
        assert cx.render_stat()["uploaded_bytes"] > 0
        same_bits(got, resident[mode])


# ---- 3. edges of the launch shapes
def strip(nv):
    """grid(n, 2) cut to exactly nv vertices (odd nv: without its last vertex and the faces that use it)"""
    m = mg.grid((nv + 1) // 2, 2)
    tris = m.indices.reshape(-1, 3)
    tris = tris[(tris < nv).all(axis=1)]
    return mg.Mesh(m.verts[:nv], np.full(len(tris), 3, np.uint8), tris.reshape(-1))


@pytest.mark.parametrize("nv", [63, 64, 65, 255, 256, 257])
def test_strips(cx, nv):
    m = strip(nv)
    assert m.nv == nv
    check(cx, mesh_of(m))


def test_single_triangle(cx):
    got = check(cx, xyz_mesh([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [3], [0, 1, 2]))
    for mode in MODES:
        assert np.array_equal(got[mode]["face_normals"], [[0, 0, 1]]) and np.array_equal(got[mode]["normals"], [[0, 0, 1]] * 3)


def test_last_face_is_the_only_heptagon(cx):
    g = mg.grid(7, 6)
    a = 2 * np.pi * np.arange(7) / 7
    ring = np.stack([3 + np.cos(a), np.sin(a), 0.05 * np.cos(3 * a)], axis=1)   # not planar
    pos = np.concatenate([nr.positions_of(g.verts), ring.astype(np.float32)])
    deg = np.concatenate([g.degrees, [7]])
    idx = np.concatenate([g.indices, g.nv + np.arange(7)])
    mesh = xyz_mesh(pos, deg, idx)
    assert mesh.ntri == g.nf + 5
    check(cx, mesh)


# ---- 4. hubs
def fans(nfans, spokes):
    """closed fans of `spokes` triangles round an apex lifted off the rim plane, side by side"""
    a = 2 * np.pi * np.arange(spokes) / spokes
    rim = np.stack([np.cos(a), np.sin(a), np.zeros(spokes)], axis=1)
    pos, idx = [], []
    for k in range(nfans):
        base = k * (spokes + 1)
        centre = np.array([3.0 * (k % 20), 3.0 * (k // 20), 0.0])
        pos.append(np.concatenate([[centre + [0, 0, 0.5]], rim + centre]))
        r = base + 1 + np.arange(spokes)
        idx.append(np.stack([np.full(spokes, base), r, base + 1 + (np.arange(spokes) + 1) % spokes], axis=1))
    idx = np.concatenate(idx).reshape(-1)
    return xyz_mesh(np.concatenate(pos), np.full(len(idx) // 3, 3, np.uint8), idx)


@pytest.mark.parametrize("nfans,spokes", [(1, 20000), (300, 100)], ids=["valence20000", "fans300x100"])
def test_hubs(cx, nfans, spokes):
    mesh = fans(nfans, spokes)
    first = check(cx, mesh)
    for mode in MODES:
        apex = first[mode]["normals"][:: spokes + 1]
        assert len(apex) == nfans and (apex[:, 2] > 0.8).all()
        same_bits(cx.render_numpy(mesh, normals=mode, face_normals=True), first[mode])


# ---- 5. exact zeros (integer-lattice coordinates: every product and sum is exact)
def test_degenerate_faces(cx):
    pos = [[0, 0, 0], [2, 0, 0], [0, 2, 0], [4, 0, 0], [2, 2, 3], [7, 7, 7]]
    # good, a repeated index, three collinear corners, good; vertex 5 is unreferenced
    mesh = xyz_mesh(pos, [3, 3, 3, 3], [0, 1, 2, 0, 1, 1, 0, 1, 3, 1, 4, 2])
    got = check(cx, mesh)
    for mode in MODES:
        fn, vn = got[mode]["face_normals"], got[mode]["normals"]
        assert np.array_equal(fn[1], [0, 0, 0]) and np.array_equal(fn[2], [0, 0, 0])
        assert np.array_equal(fn[0], [0, 0, 1]) and np.abs(fn[3]).max() > 0
        assert np.array_equal(vn[0], [0, 0, 1])            # only the good face counts at vertex 0
        assert np.array_equal(vn[3], [0, 0, 0]) and np.array_equal(vn[5], [0, 0, 0])   # only a degenerate face; unreferenced


def test_opposed_faces(cx):
    mesh = xyz_mesh([[0, 0, 0], [3, 0, 0], [0, 5, 1]], [3, 3], [0, 1, 2, 0, 2, 1])
    got = cx.render_numpy(mesh, normals="area", face_normals=True)
    assert np.array_equal(got["normals"], np.zeros((3, 3), np.float32))
    assert np.array_equal(got["face_normals"][0], -got["face_normals"][1]) and np.abs(got["face_normals"]).max() > 0


def test_nan_and_infinity(cx):
    n = 6
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    pos = np.stack([i, j, (i * j) % 3], axis=-1).reshape(-1, 3).astype(np.float32)
    pos[14, 0], pos[27, 0] = np.nan, np.inf
    idx = mg.grid(n, n).indices
    mesh = xyz_mesh(pos, np.full(len(idx) // 3, 3, np.uint8), idx)
    got = check(cx, mesh)
    tris = idx.reshape(-1, 3)
    hit = np.isin(tris, [14, 27]).any(axis=1)
    for mode in MODES:
        fn, vn = got[mode]["face_normals"], got[mode]["normals"]
        assert hit.sum() >= 8 and not fn[hit].any() and np.abs(fn[~hit]).max(axis=1).min() > 0
        assert not vn[[14, 27]].any()
        assert np.abs(np.delete(vn, [14, 27], axis=0)).max(axis=1).min() > 0   # their neighbours keep the faces that are whole


# ---- 6. unwelded
def test_unwelded_scene(cx):
    sc = og.scene(mg.torus(24, 26, polys="mixed"), normals="smooth", tex="atlas", charts=5)
    mesh = hc.Mesh.from_obj(sc.obj, "")
    plain = cx.render_numpy(mesh)
    got = check(cx, mesh)
    for mode in MODES:
        g = got[mode]
        vsrc = g["vertex_source"]
        assert len(vsrc) > mesh.nv and sorted(set(g) - set(plain)) == ["face_normals", "normals"]
        bits = g["normals"].view(np.uint32)
        per_vertex = np.zeros((mesh.nv, 3), np.uint32)
        per_vertex[vsrc] = bits
        assert np.array_equal(per_vertex[vsrc], bits)   # output vertices of one decoded vertex: identical bits
        for k in plain:   # the stored vn (and everything else) stay what they are
            assert np.array_equal(g[k].view(np.uint8), plain[k].view(np.uint8)), k
        stored = [l for l in range(mesh.nlists) if mesh.list_target(l) == 2 and len(mesh.list_fmt(l)) == 3]
        assert stored and not np.array_equal(g[f"list{stored[0]}"], g["normals"])


# ---- 7. nothing else moved
def raw_build(cx, mesh, flags):
    """every buffer of hry_render_build (flags None) or hry_render_build_ex as host bytes"""
    L = nat.load()
    r = C.c_void_p()
    nat.check(L.hry_render_build(cx.h, mesh.h, C.byref(r)) if flags is None else L.hry_render_build_ex(cx.h, mesh.h, flags, C.byref(r)))
    try:
        out = {}
        for name in hc.Codec.RENDER_FIXED + tuple(f"list{l}" for l in range(mesh.nlists)) + ("normals", "face_normals"):
            rows, width, typ = C.c_uint64(), C.c_int(), C.c_int()
            nat.check(L.hry_render_get(r, name.encode(), None, C.byref(rows), C.byref(width), C.byref(typ)))
            if rows.value:
                a = np.empty(rows.value * width.value * (2 if typ.value == 6 else 4), np.uint8)
                nat.check(L.hry_render_copy(cx.h, r, name.encode(), a.ctypes.data, 0))
                out[name] = (rows.value, width.value, typ.value, a)
        return out
    finally:
        L.hry_render_free(r)


@pytest.mark.parametrize("kind", ["ply", "obj"])
def test_flags_zero_is_render_build(cx, kind):
    mesh = hc.Mesh.from_ply(_read(os.path.join(GOLD, "torus_mixed.ply"))) if kind == "ply" else \
        hc.Mesh.from_obj(_read(os.path.join(GOLD, "obj", "smooth.obj")), os.path.join(GOLD, "obj"))
    a, b = raw_build(cx, mesh, None), raw_build(cx, mesh, 0)
    assert sorted(a) == sorted(b) and "normals" not in a and "face_normals" not in a
    for k in a:
        assert a[k][:3] == b[k][:3] and np.array_equal(a[k][3], b[k][3]), k
    keys = set(cx.render_numpy(mesh))
    assert keys == set(a)
    with_fn = raw_build(cx, mesh, FN)
    assert sorted(with_fn) == sorted(list(a) + ["face_normals"]) and with_fn["face_normals"][:3] == (mesh.nf, 3, 0)


# ---- 8. refusals
def refused(cx, mesh, flags, code, good):
    L = nat.load()
    r = C.c_void_p(1)
    assert L.hry_render_build_ex(cx.h, mesh.h, flags, C.byref(r)) == code
    assert not r.value and L.hry_last_error()
    check(cx, good, ("area",))   # the context stays usable
    return L.hry_last_error


def test_refusals(cx):
    good = xyz_mesh([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [3], [0, 1, 2])
    flat = np.zeros(3, np.dtype([("x", "<f4"), ("y", "<f4")]))
    flat["x"], flat["y"] = [0, 1, 0], [0, 0, 1]
    xy = hc.Mesh.from_arrays(flat, np.array([3], np.uint8), np.array([0, 1, 2], np.uint32))
    L = nat.load()
    r = C.c_void_p(1)
    assert L.hry_render_build_ex(cx.h, xy.h, VN, C.byref(r)) == nat.E_UNSUPPORTED
    assert not r.value and b"position" in L.hry_last_error()
    refused(cx, xy, FN, nat.E_UNSUPPORTED, good)
    assert "list1" in cx.render_numpy(xy)   # without normals the mesh renders as before
    refused(cx, good, 8, nat.E_ARG, good)
    refused(cx, good, VN | 16, nat.E_ARG, good)
    refused(cx, good, ANGLE, nat.E_ARG, good)
    refused(cx, good, ANGLE | FN, nat.E_ARG, good)
    with pytest.raises(ValueError):
        cx.render_numpy(good, normals="smooth")


def test_partial_mesh_refused(cx):
    mc = hc.MultiCodec([0])
    try:
        three = mg.concat([mg.torus(12, 14, polys="mixed", center=(4.0 * k, 0, 0)) for k in range(3)])   # a component per shard
        data = mc.write_hry(hc.Mesh.from_ply(three.to_ply()), quants=[(1, -1, 12)], n_shards=3)
        assert hc.container_info(data)["segments"] == 3
    finally:
        mc.close()
    share = cx.read_hry(data, shard=(0, 3))
    assert share.partial
    refused(cx, share, VN | FN, nat.E_ARG, xyz_mesh([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [3], [0, 1, 2]))


# ---- 9. torch
TORCH_CHILD = r"""
import sys
import numpy as np
import torch
torch.cuda.init()   # a PyTorch program: torch holds the device before the codec starts
sys.path.insert(0, sys.argv[1])
from harry_amd import codec as hc
from harry_amd import meshgen as mg
from harry_amd import objgen as og
m = mg.torus(16, 18, polys="mixed")
sc = og.scene(m, normals="smooth", tex="atlas", charts=3)
c = hc.Codec(0)
for mesh in (hc.Mesh.from_arrays(m.verts, m.degrees, m.indices), hc.Mesh.from_obj(sc.obj, "")):
    ref = c.render_numpy(mesh, normals="area", face_normals=True)
    got = c.render(mesh, normals="area", face_normals=True)
    assert sorted(got) == sorted(ref), (sorted(got), sorted(ref))
    U = len(ref["vertex_source"])
    for k, shape in (("normals", (U, 3)), ("face_normals", (mesh.nf, 3))):
        t = got[k]
        assert t.device == torch.device("cuda", 0) and t.dtype == torch.float32 and tuple(t.shape) == shape, k
        assert np.array_equal(t.cpu().numpy().view(np.uint32), ref[k].view(np.uint32)), k
    assert sorted(c.render(mesh)) == sorted(c.render_numpy(mesh)) and "normals" not in c.render(mesh)
c.close()
print("torch ok")
"""


def test_torch_tensors():
    """Codec.render with normals in a fresh process that uses torch first: float32 cuda tensors [U, 3] and [nf, 3], equal to
    render_numpy's"""
    import subprocess
    import sys
    pytest.importorskip("torch")
    r = subprocess.run([sys.executable, "-c", TORCH_CHILD, util.ROOT], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "torch ok" in r.stdout, r.stdout + r.stderr
