"""Meshes from device buffers (include/harry_amd.h: hry_mesh_from_device; kernels: harry_amd/csrc/device/ingest.hip) through
Codec.mesh_from_tensors: the same containers as Mesh.from_arrays of the same values, the exact weld against tests/ingest_ref.py,
the round trip with Codec.render, residency on the context, the refusals, and torch's stream."""
import ctypes as C

import numpy as np
import pytest

from harry_amd import _native as nat
from harry_amd import codec as hc
from harry_amd import meshgen as mg
from tests import ingest_ref as ir

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DEV = torch.device("cuda", 0)
POS_Q = [(1, 0, 14), (1, 1, 14), (1, 2, 14)]
NRM_Q = [(1, 3, 10), (1, 4, 10), (1, 5, 10)]


@pytest.fixture(scope="module")
def cx():
    c = hc.Codec(0)
    yield c
    c.close()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def spec_of(struct, group_xyz=True):
    """[(names, tensor)] of a structured array: x y z as one [n, 3] tensor, every other field a column of its own"""
    if struct is None:
        return None
    names = list(struct.dtype.names)
    out = []
    if group_xyz and names[:3] == ["x", "y", "z"]:
        out.append(("x y z", _t(np.stack([struct[k] for k in "xyz"], axis=1))))
        names = names[3:]
    out += [(k, _t(struct[k])) for k in names]
    return out


def ingest(cx, m: mg.Mesh, **kw):
    tri = bool((m.degrees == 3).all())
    if tri and not kw.pop("force_degrees", False):
        return cx.mesh_from_tensors(_t(m.indices.astype(np.int32).reshape(-1, 3)), spec_of(m.verts), faces=spec_of(m.face_props), **kw)
    return cx.mesh_from_tensors(_t(m.indices.astype(np.int64)), spec_of(m.verts), faces=spec_of(m.face_props), degrees=_t(m.degrees), **kw)


def host(m: mg.Mesh):
    return hc.Mesh.from_arrays(m.verts, m.degrees, m.indices, m.face_props)


def quant_of(m: mg.Mesh):
    return POS_Q + (NRM_Q if "nx" in m.verts.dtype.names else [])


def hub_fan(n=60, seed=3):
    """a cone: vertex 0 shared by n triangles (2n half-edges in its segment: above twins.hip's kTwinSegMax, matched on the host)"""
    rng = np.random.default_rng(seed)
    a = 2 * np.pi * np.arange(n) / n
    v = np.zeros(n + 1, np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4")]))
    v["x"][1:], v["y"][1:] = np.cos(a), np.sin(a)
    v["z"] = rng.normal(0, 1e-3, n + 1).astype(np.float32)
    v["z"][0] = 0.5
    ring = np.arange(1, n + 1)
    tris = np.stack([np.zeros(n, np.int64), ring, ring % n + 1], 1).astype(np.uint32)
    return mg.Mesh(v, np.full(n, 3, np.uint8), tris.reshape(-1))


MESHES = {
    "torus_normals": lambda: mg.torus(24, 26, normals=True),
    "multi_mixed": lambda: mg.multi_component(3, 10, 12, polys="mixed"),
    "colors": lambda: mg.with_colors(mg.torus(14, 16, polys="quad")),
    "face_props": lambda: mg.with_face_props(mg.torus(12, 14, polys="mixed", normals=True)),
    "nonmanifold": lambda: mg.with_nonmanifold(mg.torus(16, 18, polys="mixed"), 4, 2),
    "hub_fan": hub_fan,
}


# ---- 1. byte-identical containers, and the same arrays as the host-built mesh after its upload
@pytest.mark.parametrize("name", sorted(MESHES))
def test_same_containers_as_from_arrays(cx, name):
    m = MESHES[name]()
    for profile in (hc.PROFILE_COMPAT, hc.PROFILE_CHUNKED):
        for quant in ([], quant_of(m)):
            a, b = ingest(cx, m), host(m)
            if quant:
                cx.requant(a, quant)
                cx.requant(b, quant)
            assert cx.write_hry(a, profile=profile) == cx.write_hry(b, profile=profile), (name, profile, quant)
    a = ingest(cx, m)
    assert cx.resident(a)
    other = hc.Codec(0)
    try:
        b = host(m)
        other.upload(b)
        assert (a.nv, a.nf, a.ne) == (b.nv, b.nf, b.ne)
        for get in ("org", "twin", "face_offsets"):
            assert np.array_equal(getattr(a, get)(), getattr(b, get)()), get
        for l in range(2):
            assert a.list_fmt(l) == b.list_fmt(l)
            assert np.array_equal(a.list_data(l), b.list_data(l)), l
    finally:
        other.close()


def test_degrees_path_for_triangles(cx):
    m = mg.torus(20, 22, normals=True)
    a, b = ingest(cx, m, force_degrees=True), host(m)
    assert cx.write_hry(a) == cx.write_hry(b)


def test_strided_views(cx):
    """columns of one interleaved [n, 6] tensor, and of a transposed one: no copy, the same mesh"""
    m = mg.torus(18, 20, normals=True)
    names = list(m.verts.dtype.names)
    full = _t(np.stack([m.verts[k] for k in names], axis=1))
    idx = _t(m.indices.astype(np.int32).reshape(-1, 3))
    want = cx.write_hry(host(m))
    assert cx.write_hry(cx.mesh_from_tensors(idx, [(" ".join(names), full)])) == want
    tr = full.t().contiguous().t()   # column-major view
    assert not tr.is_contiguous()
    assert cx.write_hry(cx.mesh_from_tensors(idx, [("x y z", tr[:, :3]), ("nx ny nz", tr[:, 3:])])) == want


# ---- 2. weld
def soup_of(m: mg.Mesh, seed=1):
    """three rows per triangle, triangles shuffled: (positions [3T, 3] float32, soup indices [T, 3])"""
    tris = m.indices.reshape(-1, 3)[np.random.default_rng(seed).permutation(m.nf)]
    pos = np.stack([m.verts[k] for k in "xyz"], axis=1)[tris.reshape(-1)]
    return pos, np.arange(3 * m.nf, dtype=np.int32).reshape(-1, 3)


def check_weld(cx, m: mg.Mesh, compare_container=True):
    pos, sidx = soup_of(m)
    mesh, remap = cx.mesh_from_tensors(_t(sidx), [("x y z", _t(pos))], weld=True, return_remap=True)
    want_remap, first = ir.weld(ir.packed_records([pos[:, 0], pos[:, 1], pos[:, 2]]))
    assert mesh.nv == len(first) == m.nv
    assert remap.dtype == torch.int32 and remap.device == DEV
    assert np.array_equal(remap.cpu().numpy().view(np.uint32), want_remap)
    if compare_container:
        verts = np.zeros(len(first), m.verts.dtype)
        for j, k in enumerate("xyz"):
            verts[k] = pos[first, j]
        welded = hc.Mesh.from_arrays(verts, np.full(m.nf, 3, np.uint8), want_remap[sidx.reshape(-1)])
        assert cx.write_hry(mesh) == cx.write_hry(welded)
    return mesh


def test_weld_shuffled_soup(cx):
    check_weld(cx, mg.torus(30, 34))


def test_weld_soup_configs1_size(cx):
    m = mg.torus(708, 708, seed=2, sigma=1e-4)   # configs[1]: 3 007 584 soup rows
    check_weld(cx, m, compare_container=False)


def test_weld_keeps_faces_and_unreferenced_rows(cx):
    # rows 0 and 2 equal, row 4 unreferenced, the second face collapses to (0, 0, 1) after the weld: kept as it is
    x = np.array([0.0, 1.0, 0.0, 0.0, 7.0], np.float32)
    y = np.array([0.0, 0.0, 0.0, 1.0, 7.0], np.float32)
    idx = np.array([[0, 1, 3], [0, 2, 1]], np.int32)
    mesh, remap = cx.mesh_from_tensors(_t(idx), [("x", _t(x)), ("y", _t(y))], weld=True, return_remap=True)
    assert remap.cpu().tolist() == [0, 1, 0, 2, 3] and mesh.nv == 4 and mesh.nf == 2
    assert mesh.org().tolist() == [0, 1, 2, 0, 0, 1]
    v = np.zeros(4, np.dtype([("x", "<f4"), ("y", "<f4")]))
    v["x"], v["y"] = x[[0, 1, 3, 4]], y[[0, 1, 3, 4]]
    want = hc.Mesh.from_arrays(v, np.full(2, 3, np.uint8), np.array([0, 1, 2, 0, 0, 1], np.uint32))
    assert np.array_equal(mesh.list_data(1), want.list_data(1)) and np.array_equal(mesh.twin(), want.twin())


def test_weld_signed_zero_and_nan(cx):
    x = np.array([0x00000000, 0x80000000, 0x7FC00000, 0x7FC00001, 0x7FC00000, 0x00000000], np.uint32).view(np.float32)
    idx = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    _, remap = cx.mesh_from_tensors(_t(idx), [("x", _t(x))], weld=True, return_remap=True)
    assert remap.cpu().tolist() == [0, 1, 2, 3, 2, 0]


# The edges of the shared first-occurrence numbering (dedup.hip): fewer rows than a wavefront, one row either side of a wavefront
# and of a block of 256, and 65 601 rows -- 1026 wavefront counts, so every thread of the one-block scan takes more than one.
# "distinct": every probe claims a slot.  "tail_equal": rows 0, 1, 2 distinct and every later row equal to row 2, so n - 2 lanes
# meet in one slot (the losers of the compare-and-swap, then atomicMin); the rows past 2 are unreferenced, the face is (0, 1, 2).
@pytest.mark.parametrize("pattern", ["distinct", "tail_equal"])
@pytest.mark.parametrize("n", [3, 63, 64, 65, 256, 257, 65601])
def test_weld_numbering_edges(cx, n, pattern):
    x = np.arange(n, dtype=np.float32)
    if pattern == "tail_equal":
        x[3:] = x[2]
    want_remap, first = ir.weld(ir.packed_records([x]))
    assert len(first) == (n if pattern == "distinct" else 3)
    mesh, remap = cx.mesh_from_tensors(_t(np.array([[0, 1, 2]], np.int32)), [("x", _t(x))], weld=True, return_remap=True)
    assert mesh.nv == len(first)
    assert np.array_equal(remap.cpu().numpy().view(np.uint32), want_remap)


# ---- 3. round trip with render
def test_round_trip_with_render(cx):
    m = mg.torus(26, 28)
    dec = cx.read_hry(cx.write_hry(host(m)))
    buf = cx.render(dec)
    mesh = cx.mesh_from_tensors(buf["indices"], [("x y z", buf["list1"])])
    assert cx.write_hry(mesh) == cx.write_hry(dec)


# ---- 4. residency
def test_residency(cx):
    m, other_m = mg.torus(22, 24, normals=True), mg.torus(9, 11)
    want = cx.write_hry(host(m), profile=hc.PROFILE_CHUNKED)
    mesh = ingest(cx, m)
    assert cx.resident(mesh)
    second = hc.Codec(0)
    try:
        assert not second.resident(mesh)
        assert second.write_hry(mesh, profile=hc.PROFILE_CHUNKED) == want
    finally:
        second.close()
    mesh = ingest(cx, m)
    cx.upload(host(other_m))
    assert not cx.resident(mesh)
    assert cx.write_hry(mesh, profile=hc.PROFILE_CHUNKED) == want


# ---- 5. refusals: code and text, *out stays NULL, the context still encodes
def refused(cx, code, text, fn):
    with pytest.raises(hc.HryError) as e:
        fn()
    assert e.value.code == code, (e.value.code, e.value.msg)
    assert text in e.value.msg, e.value.msg
    m = mg.torus(8, 9)
    assert cx.write_hry(ingest(cx, m)) == cx.write_hry(host(m))


def test_refusals(cx):
    m = mg.torus(10, 12)
    pos = [("x y z", _t(np.stack([m.verts[k] for k in "xyz"], axis=1)))]
    tri = m.indices.astype(np.int64).reshape(-1, 3)
    bad = tri.copy()
    bad[5, 1] = m.nv
    refused(cx, nat.E_ARG, "vertex index out of range", lambda: cx.mesh_from_tensors(_t(bad), pos))
    bad = tri.copy()
    bad[7, 2] = -1
    refused(cx, nat.E_ARG, "vertex index out of range", lambda: cx.mesh_from_tensors(_t(bad), pos))
    for d in (2, 0):
        deg = np.full(m.nf, 3, np.uint8)
        deg[3] = d
        deg[4] = 3 + (3 - d)   # (the sum still matches)
        refused(cx, nat.E_UNSUPPORTED, "polygon degree outside 3..255",
                lambda: cx.mesh_from_tensors(_t(tri.reshape(-1)), pos, degrees=_t(deg)))
    deg = np.full(m.nf, 3, np.uint8)
    refused(cx, nat.E_ARG, "sum of degrees", lambda: cx.mesh_from_tensors(_t(tri.reshape(-1)[:-1]), pos, degrees=_t(deg)))
    refused(cx, nat.E_ARG, "not a tensor on", lambda: cx.mesh_from_tensors(torch.from_numpy(tri), pos))
    # through the C ABI: a host pointer, *out stays NULL
    host_pos = np.ascontiguousarray(np.stack([m.verts[k] for k in "xyz"], axis=1))
    cols = (nat.DevColumn * 3)(*[nat.DevColumn(host_pos.ctypes.data + 4 * j, 12, n.encode(), 0) for j, n in enumerate("xyz")])
    idx = _t(tri.astype(np.int32))
    out = C.c_void_p(1)
    rc = nat.load().hry_mesh_from_device(cx.h, m.nv, cols, 3, m.nf, None, idx.data_ptr(), 4, idx.numel(), None, 0, 0, None, C.byref(out))
    assert rc == nat.E_ARG and not out.value
    assert "not device memory" in nat.load().hry_last_error().decode()
    assert cx.write_hry(ingest(cx, m)) == cx.write_hry(host(m))


def test_refusal_other_device(cx):
    """a tensor on another device: the binding refuses it, and so does the library past the binding's own check"""
    if torch.cuda.device_count() < 2:
        pytest.skip("one device visible")
    m = mg.torus(10, 12)
    on1 = torch.from_numpy(np.stack([m.verts[k] for k in "xyz"], axis=1).copy()).to(torch.device("cuda", 1))
    refused(cx, nat.E_ARG, "not a tensor on", lambda: cx.mesh_from_tensors(_t(m.indices.astype(np.int32).reshape(-1, 3)), [("x y z", on1)]))
    cols = (nat.DevColumn * 3)(*[nat.DevColumn(on1.data_ptr() + 4 * j, 12, n.encode(), 0) for j, n in enumerate("xyz")])
    idx = _t(m.indices.astype(np.int32))
    out = C.c_void_p(1)
    rc = nat.load().hry_mesh_from_device(cx.h, m.nv, cols, 3, m.nf, None, idx.data_ptr(), 4, idx.numel(), None, 0, 0, None, C.byref(out))
    assert rc == nat.E_ARG and not out.value
    assert cx.write_hry(ingest(cx, m)) == cx.write_hry(host(m))


# ---- 6. torch's stream
def test_stream_contract(cx):
    m = mg.torus(60, 64, normals=True)
    pos = _t(np.stack([m.verts[k] for k in "xyz"], axis=1))
    nrm = _t(np.stack([m.verts[k] for k in ("nx", "ny", "nz")], axis=1))
    idx = _t(m.indices.astype(np.int32).reshape(-1, 3))
    want = cx.write_hry(cx.mesh_from_tensors(idx, [("x y z", pos), ("nx ny nz", nrm)]))
    for _ in range(3):
        p2, n2, i2 = pos * 1.0, nrm * 1.0, idx + 0   # written by torch kernels on its stream right before the call
        assert cx.write_hry(cx.mesh_from_tensors(i2, [("x y z", p2), ("nx ny nz", n2)])) == want
