"""Textured meshes from device buffers (include/harry_amd.h: hry_mesh_from_device_corners; kernels: harry_amd/csrc/device/ingest.hip)
through Codec.corner_mesh_from_tensors: the same mesh and the same containers as Mesh.from_obj of the same arrays, the region
numbering and the per-list weld against tests/ingest_corners_ref.py, the round trip with Codec.render, residency on the context, the
refusals, and torch's stream.

The scenes are objgen scenes over mg.torus(24, 26): 624 vertices, 1 248 triangles or 970 mixed polygons -- more than one 256-lane
block per kernel, and row and corner counts that are no multiples of 64."""
import ctypes as C

import numpy as np
import pytest

from harry_amd import _native as nat
from harry_amd import codec as hc
from harry_amd import meshgen as mg
from harry_amd import objgen as og
from tests import ingest_corners_ref as icr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DEV = torch.device("cuda", 0)

SCENES = {
    "atlas_smooth_mat3": dict(tex="atlas", normals="smooth", charts=5, materials=3),
    "tex_only": dict(tex="atlas", charts=5),
    "normals_only_flat": dict(normals="flat"),
    "tex3": dict(tex="atlas", charts=5, tex3=True, normals="smooth"),
    "neither": dict(),
}


@pytest.fixture(scope="module")
def cx():
    c = hc.Codec(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def other():
    c = hc.Codec(0)
    yield c
    c.close()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def scene_of(polys="tri", **kw):
    return og.scene(mg.torus(24, 26, polys=polys), **kw)


def load(sc, tmp_path):
    for name, data in sc.files.items():
        (tmp_path / name).write_bytes(data)
    return hc.Mesh.from_obj(sc.obj, str(tmp_path))


def arrays_of(ref, tex, nrm):
    """the reader's own arrays: rows of every list (float32), the row every corner names in it, degrees, the faces' regions"""
    def rows(l):
        return ref.list_data(l).view(np.float32).copy()
    cattr = ref.bindings(2)
    a = {"pos": rows(0), "pos_idx": ref.org().astype(np.int64), "uv": None, "uv_idx": None, "nrm": None, "nrm_idx": None,
         "degrees": np.diff(ref.face_offsets().astype(np.int64)).astype(np.uint8), "materials": ref.regions_of(0).copy()}
    l = 1
    if tex:
        a["uv"], a["uv_idx"] = rows(l), cattr[:, l - 1].astype(np.int64)
        l += 1
    if nrm:
        a["nrm"], a["nrm_idx"] = rows(l), cattr[:, l - 1].astype(np.int64)
    return a


def build(cx, a, force_degrees=False, materials=True, **kw):
    tri = bool((a["degrees"] == 3).all()) and not force_degrees

    def idx(x):
        return None if x is None else _t(x.astype(np.int32).reshape(-1, 3)) if tri else _t(x.astype(np.int64))

    def rows(x):
        return None if x is None else _t(x)
    mat = _t(a["materials"].view(np.int16)) if materials and a["materials"] is not None else None
    return cx.corner_mesh_from_tensors(rows(a["pos"]), idx(a["pos_idx"]), uv=rows(a["uv"]), uv_idx=idx(a["uv_idx"]), normals=rows(a["nrm"]),
                                       normal_idx=idx(a["nrm_idx"]), degrees=None if tri else _t(a["degrees"]), materials=mat, **kw)


def quant_of(tex, nrm):
    q, l = [(0, -1, 14)], 1
    if tex:
        q.append((l, -1, 10))
        l += 1
    if nrm:
        q.append((l, -1, 10))
    return q


def same_mesh(a, b):
    assert (a.nv, a.nf, a.ne, a.nlists) == (b.nv, b.nf, b.ne, b.nlists)
    assert a.general and b.general
    for get in ("org", "twin", "face_offsets"):
        assert np.array_equal(getattr(a, get)(), getattr(b, get)()), get
    for l in range(b.nlists):
        assert a.list_fmt(l) == b.list_fmt(l) and a.list_target(l) == b.list_target(l), l
        assert np.array_equal(a.list_data(l), b.list_data(l)), l
    for which in (0, 1):
        assert a.nregions(which) == b.nregions(which)
        assert np.array_equal(a.regions_of(which), b.regions_of(which)), which
    for r in range(b.nregions(0)):
        for kind in (0, 2):
            assert a.region_lists(kind, r) == b.region_lists(kind, r), (kind, r)
    for r in range(b.nregions(1)):
        assert a.region_lists(1, r) == b.region_lists(1, r), r
    for kind in (1, 2):
        assert np.array_equal(a.bindings(kind), b.bindings(kind)), kind
    assert a.bindings(0).shape == b.bindings(0).shape


def containers(cx, make, quant=None):
    """[compat, chunked] of a mesh made afresh for each (a requant changes the mesh)"""
    out = []
    for profile in (hc.PROFILE_COMPAT, hc.PROFILE_CHUNKED):
        m = make()
        if quant:
            cx.requant(m, quant)
        out.append(cx.write_hry(m, profile=profile))
    return out


# ---- 1. the mesh and the containers of the OBJ reader
@pytest.mark.parametrize("polys", ["tri", "mixed"])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_equal_to_the_obj_reader(cx, other, tmp_path, name, polys):
    kw = SCENES[name]
    tex, nrm = "tex" in kw, "normals" in kw
    sc = scene_of(polys, **kw)
    ref = load(sc, tmp_path)
    a = arrays_of(ref, tex, nrm)
    got = build(cx, a)
    assert cx.resident(got)
    other.upload(ref)
    same_mesh(got, ref)
    assert got.to_obj() == ref.to_obj()
    for quant in (None, quant_of(tex, nrm)):
        assert containers(cx, lambda: build(cx, a), quant) == containers(cx, lambda: load(sc, tmp_path), quant), (name, polys, quant)


# ---- 2. int64 indices with degrees on an all-triangle scene
def test_int64_indices_with_degrees(cx, tmp_path):
    a = arrays_of(load(scene_of(**SCENES["atlas_smooth_mat3"]), tmp_path), True, True)
    assert containers(cx, lambda: build(cx, a, force_degrees=True)) == containers(cx, lambda: build(cx, a))


# ---- 3. face regions: the distinct materials in order of first occurrence
def test_region_numbering(cx, tmp_path):
    a = arrays_of(load(scene_of(tex="atlas", charts=5, normals="smooth"), tmp_path), True, True)
    nf = len(a["degrees"])
    bounds = [0, 64, 100, 128, 129, 700, 1000, nf]   # runs: a boundary at multiples of 64, a run of one face
    values = [900, 65535, 3, 900, 0, 17, 65535]      # not sorted, repeated, the largest u16
    mat = np.zeros(nf, np.uint16)
    for i, v in enumerate(values):
        mat[bounds[i]:bounds[i + 1]] = v
    a["materials"] = mat
    got = build(cx, a)
    want = icr.regions_by_first_occurrence(mat)
    assert got.nregions(0) == 5 and np.array_equal(got.regions_of(0), want)
    assert want[[0, 64, 100, 128, 129, 700, 1000]].tolist() == [0, 1, 2, 0, 3, 4, 1]
    for r in range(5):
        assert got.region_lists(2, r) == [1, 2]
    # the limit: 128 distinct values pass, 129 do not
    a["materials"] = ((np.arange(nf) * 7919) % 128 * 509 + 11).astype(np.uint16)
    got = build(cx, a)
    assert got.nregions(0) == 128 and np.array_equal(got.regions_of(0), icr.regions_by_first_occurrence(a["materials"]))
    a["materials"] = ((np.arange(nf) * 7919) % 129 * 503 + 11).astype(np.uint16)
    assert len(np.unique(a["materials"])) == 129
    with pytest.raises(hc.HryError) as e:
        build(cx, a)
    assert e.value.code == nat.E_UNSUPPORTED and "more than 128 regions" in e.value.msg


# ---- 4. strided views of one interleaved tensor
def test_strided_views(cx, tmp_path):
    a = arrays_of(load(scene_of(**SCENES["atlas_smooth_mat3"]), tmp_path), True, True)
    table = np.concatenate([a["pos"][a["pos_idx"]], a["uv"][a["uv_idx"]], a["nrm"][a["nrm_idx"]]], axis=1)   # one row per corner
    assert table.shape[1] == 8
    full = _t(table)
    idx = _t(np.arange(len(table), dtype=np.int32).reshape(-1, 3))
    mat = _t(a["materials"].view(np.int16))
    views = (full[:, 0:3], full[:, 3:5], full[:, 5:8])
    assert not any(v.is_contiguous() for v in views)
    want = [cx.write_hry(cx.corner_mesh_from_tensors(views[0].contiguous(), idx, uv=views[1].contiguous(), normals=views[2].contiguous(),
                                                     materials=mat, weld=w)) for w in (False, True)]
    got = [cx.write_hry(cx.corner_mesh_from_tensors(views[0], idx, uv=views[1], normals=views[2], materials=mat, weld=w)) for w in (False, True)]
    assert got == want and got[0] != got[1]


# ---- 5. weld: every list on its own
def check_against_restatement(cx, mesh, remaps, a, e):
    ne = len(a["pos_idx"])
    for k, name in enumerate(("pos", "uv", "nrm")):
        if a[name] is None:
            assert remaps[k] is None
            continue
        assert remaps[k].dtype == torch.int32 and remaps[k].device == DEV
        assert np.array_equal(remaps[k].cpu().numpy().view(np.uint32), e["remaps"][k]), name
    given = [x for x in e["lists"] if x is not None]
    assert mesh.nlists == len(given) and mesh.nv == len(given[0])
    for l, rows in enumerate(given):
        assert mesh.list_count(l) == len(rows)
        assert np.array_equal(mesh.list_data(l), np.ascontiguousarray(rows).view(np.uint8).reshape(len(rows), -1)), l
    assert np.array_equal(mesh.org(), e["org"])
    assert np.array_equal(mesh.bindings(2), e["corner_attr"].reshape(ne, 2))
    assert np.array_equal(mesh.bindings(1), e["vtx_attr"])


def test_weld(cx, tmp_path):
    a = arrays_of(load(scene_of(tex="corner", normals="smooth"), tmp_path), True, True)
    assert len(a["uv"]) == 3744 and len(np.unique(a["uv"].view(np.uint64))) == 702   # the corner texture coordinates repeat already
    rng = np.random.default_rng(5)
    for rows, idx in (("pos", "pos_idx"), ("nrm", "nrm_idx")):   # a shuffled copy of the rows; half of the corners name the copies
        n = len(a[rows])
        perm = rng.permutation(n)
        where = np.empty(n, np.int64)
        where[perm] = n + np.arange(n)
        a[rows] = np.concatenate([a[rows], a[rows][perm]])
        half = rng.random(len(a[idx])) < 0.5
        a[idx] = np.where(half, where[a[idx]], a[idx])
    a["pos"] = np.concatenate([a["pos"], np.array([[9, 9, 9]], np.float32)])   # a row no corner names
    mesh, remaps = build(cx, a, weld=True, return_remap=True)
    e = icr.expected(a["pos"], a["pos_idx"], a["uv"], a["uv_idx"], a["nrm"], a["nrm_idx"], weld=True)
    assert (len(e["lists"][0]), len(e["lists"][1]), len(e["lists"][2])) == (625, 702, 624)
    check_against_restatement(cx, mesh, remaps, a, e)
    assert not (mesh.org() == 624).any() and mesh.nv == 625   # the unreferenced row stays a vertex
    welded = dict(a, pos=e["lists"][0], uv=e["lists"][1], nrm=e["lists"][2], pos_idx=e["org"].astype(np.int64),
                  uv_idx=e["corner_attr"][:, 0].astype(np.int64), nrm_idx=e["corner_attr"][:, 1].astype(np.int64))
    assert containers(cx, lambda: build(cx, a, weld=True)) == containers(cx, lambda: build(cx, welded))
    _, ident = build(cx, welded, return_remap=True)   # without the weld: the identity
    assert [r.cpu().tolist() == list(range(len(r))) for r in ident] == [True] * 3


def test_weld_signed_zero_and_nan_in_a_uv_column(cx):
    u = np.array([0x00000000, 0x80000000, 0x7FC00000, 0x7FC00001, 0x7FC00000, 0x00000000], np.uint32).view(np.float32)
    uv = np.stack([u, np.full(6, 0.25, np.float32)], axis=1)
    pos = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], np.float32)
    idx = _t(np.array([[0, 1, 2], [2, 1, 3]], np.int32))
    mesh, remaps = cx.corner_mesh_from_tensors(_t(pos), idx, uv=_t(uv), uv_idx=_t(np.arange(6, dtype=np.int32).reshape(2, 3)), weld=True,
                                               return_remap=True)
    assert remaps[1].cpu().tolist() == [0, 1, 2, 3, 2, 0] and remaps[0].cpu().tolist() == [0, 1, 2, 3] and remaps[2] is None
    assert mesh.list_count(1) == 4 and mesh.bindings(2)[:, 0].tolist() == [0, 1, 2, 3, 2, 0]
    assert mesh.list_data(1).view(np.uint32)[:, 0].tolist() == [0x00000000, 0x80000000, 0x7FC00000, 0x7FC00001]


# ---- 6. a hub: the twins of a vertex with more half-edges than the device matches come from the host, as in an upload
def test_hub(cx, other, tmp_path):
    n = 60
    ang = 2 * np.pi * np.arange(n) / n
    v = np.zeros(n + 1, np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4")]))
    v["x"][1:], v["y"][1:] = np.cos(ang), np.sin(ang)
    v["z"][0] = 0.5
    ring = np.arange(1, n + 1)
    tris = np.stack([np.zeros(n, np.int64), ring, ring % n + 1], 1).astype(np.uint32)
    sc = og.scene(mg.Mesh(v, np.full(n, 3, np.uint8), tris.reshape(-1)), tex="corner")
    ref = load(sc, tmp_path)
    assert int((ref.org() == 0).sum()) == 60   # (120 half-edges in the apex' segment: above twins.hip's kTwinSegMax of 48)
    got = build(cx, arrays_of(ref, True, False))
    other.upload(ref)
    same_mesh(got, ref)
    assert cx.write_hry(got, profile=hc.PROFILE_CHUNKED) == other.write_hry(ref, profile=hc.PROFILE_CHUNKED)


# ---- 7. round trip with render: the weld inverts the render build's unweld
def first_occurrence(x):
    return icr.regions_by_first_occurrence(x.cpu().numpy().astype(np.int64))


def test_round_trip_with_render(cx, tmp_path):
    ref = load(scene_of(**SCENES["atlas_smooth_mat3"]), tmp_path)
    dec = cx.read_hry(cx.write_hry(ref, profile=hc.PROFILE_CHUNKED))
    buf = cx.render(dec)
    for l in range(dec.nlists):   # no list holds two equal records: the weld then gives back exactly the decoded lists' sizes
        rec = dec.list_data(l)
        assert len(np.unique(rec.view(np.dtype((np.void, rec.shape[1]))))) == len(rec), l
    tri_mat = buf["face_region"][buf["tri_face"].long()]
    m2 = cx.corner_mesh_from_tensors(buf["list0"], buf["indices"], uv=buf["list1"], normals=buf["list2"], materials=tri_mat, weld=True)
    buf2 = cx.render(m2)
    for k in ("indices", "list0", "list1", "list2"):
        assert torch.equal(buf2[k], buf[k]), k
    assert m2.nv == dec.nv
    assert np.array_equal(first_occurrence(buf2["face_region"][buf2["tri_face"].long()]), first_occurrence(tri_mat))
    for profile in (hc.PROFILE_COMPAT, hc.PROFILE_CHUNKED):
        back = cx.read_hry(cx.write_hry(m2, profile=profile))
        assert (back.nv, back.nf, back.ne, back.nlists) == (m2.nv, m2.nf, m2.ne, 3)


# ---- 8. residency
def test_residency(cx, other, tmp_path):
    sc = scene_of(**SCENES["atlas_smooth_mat3"])
    ref = load(sc, tmp_path)
    a = arrays_of(ref, True, True)
    for profile in (hc.PROFILE_COMPAT, hc.PROFILE_CHUNKED):
        want = cx.write_hry(load(sc, tmp_path), profile=profile)
        mesh = build(cx, a)
        assert cx.resident(mesh) and not other.resident(mesh)
        assert cx.write_hry(mesh, profile=profile) == want
        assert cx.resident(mesh)
        mesh = build(cx, a)
        assert other.write_hry(mesh, profile=profile) == want
        mesh = build(cx, a)
        cx.upload(hc.Mesh.from_obj(scene_of("mixed", normals="flat").obj, ""))
        assert not cx.resident(mesh)
        assert cx.write_hry(mesh, profile=profile) == want


# ---- 9. refusals: code and text, *out stays NULL, the context still encodes
@pytest.fixture(scope="module")
def small(tmp_path_factory):
    sc = og.scene(mg.torus(8, 9), tex="atlas", normals="smooth", materials=2)
    d = tmp_path_factory.mktemp("small")
    ref = load(sc, d)
    return arrays_of(ref, True, True), sc, d


def refused(cx, small, code, text, fn):
    with pytest.raises(hc.HryError) as e:
        fn()
    assert e.value.code == code, (e.value.code, e.value.msg)
    assert text in e.value.msg, e.value.msg
    a, sc, d = small
    assert cx.write_hry(build(cx, a)) == cx.write_hry(load(sc, d))


def test_refusals(cx, small):
    a = small[0]
    for key, text in (("pos_idx", "vertex index out of range"), ("uv_idx", "texture index out of range"), ("nrm_idx", "normal index out of range")):
        rows = len(a[{"pos_idx": "pos", "uv_idx": "uv", "nrm_idx": "nrm"}[key]])
        for at, value in ((70, rows), (5, -1)):
            bad = dict(a)
            bad[key] = a[key].copy()
            bad[key][at] = value
            refused(cx, small, nat.E_ARG, text, lambda: build(cx, bad, force_degrees=True))
        bad[key][5] = rows + 7
        refused(cx, small, nat.E_ARG, text, lambda: build(cx, bad, weld=True))   # int32 [T, 3], through the weld's map
    refused(cx, small, nat.E_ARG, "3, 4, 6, 7 or 8 components", lambda: build(cx, dict(a, pos=np.concatenate([a["pos"], a["pos"][:, :2]], axis=1))))
    refused(cx, small, nat.E_ARG, "float32", lambda: cx.corner_mesh_from_tensors(_t(a["pos"].astype(np.float64)), _t(a["pos_idx"].astype(np.int32).reshape(-1, 3))))
    deg = a["degrees"].copy()
    deg[3], deg[4] = 2, 4   # (the sum still matches)
    refused(cx, small, nat.E_UNSUPPORTED, "polygon degree outside 3..255", lambda: build(cx, dict(a, degrees=deg)))
    short = dict(a, pos_idx=a["pos_idx"][:-1], uv_idx=a["uv_idx"][:-1], nrm_idx=a["nrm_idx"][:-1])
    refused(cx, small, nat.E_ARG, "sum of degrees", lambda: build(cx, short, force_degrees=True))
    refused(cx, small, nat.E_ARG, "not a tensor on",
            lambda: cx.corner_mesh_from_tensors(_t(a["pos"]), torch.from_numpy(a["pos_idx"].astype(np.int32).reshape(-1, 3))))
    refused(cx, small, nat.E_ARG, "not a tensor on",
            lambda: cx.corner_mesh_from_tensors(_t(a["pos"]), _t(a["pos_idx"].astype(np.int32).reshape(-1, 3)), uv=_t(a["uv"]),
                                                uv_idx=torch.from_numpy(a["uv_idx"].astype(np.int32).reshape(-1, 3))))


def test_refusals_through_the_c_abi(cx, small):
    a, sc, d = small
    L = nat.load()
    idx = _t(a["pos_idx"].astype(np.int32))
    nf = len(a["degrees"])
    dev_pos = _t(a["pos"])

    def call(cols, pos=True, flags=0, index_type=4):
        rows = nat.DevRows(cols, 3, len(a["pos"]), idx.data_ptr())
        out = C.c_void_p(1)
        rc = L.hry_mesh_from_device_corners(cx.h, C.byref(rows) if pos else None, None, None, nf, None, index_type, idx.numel(), None, flags, None, C.byref(out))
        assert not out.value
        return rc, L.hry_last_error().decode()
    good = (nat.DevColumn * 3)(*[nat.DevColumn(dev_pos.data_ptr() + 4 * j, 12, None, 0) for j in range(3)])
    host_pos = np.ascontiguousarray(a["pos"])
    rc, msg = call((nat.DevColumn * 3)(*[nat.DevColumn(host_pos.ctypes.data + 4 * j, 12, None, 0) for j in range(3)]))
    assert rc == nat.E_ARG and "not device memory" in msg
    rc, msg = call((nat.DevColumn * 3)(*[nat.DevColumn(dev_pos.data_ptr() + 4 * j, 12, None, 1 if j == 1 else 0) for j in range(3)]))
    assert rc == nat.E_ARG and "HRY_FLOAT" in msg
    rc, msg = call((nat.DevColumn * 3)(*[nat.DevColumn(dev_pos.data_ptr() + 4 * j, 0 if j == 2 else 12, None, 0) for j in range(3)]))
    assert rc == nat.E_ARG and "stride" in msg
    rc, msg = call((nat.DevColumn * 3)(*[nat.DevColumn(dev_pos.data_ptr() + 4 * j + (2 if j == 0 else 0), 12, None, 0) for j in range(3)]))
    assert rc == nat.E_ARG and "misaligned" in msg
    assert call(good, pos=False)[0] == nat.E_ARG
    rc, msg = call(good, flags=2)
    assert rc == nat.E_ARG and "unknown flags" in msg
    rc, msg = call(good, index_type=5)
    assert rc == nat.E_ARG and "index type" in msg
    assert cx.write_hry(build(cx, a)) == cx.write_hry(load(sc, d))


# ---- 10. torch's stream
def test_stream_contract(cx, tmp_path):
    a = arrays_of(load(og.scene(mg.torus(60, 64), tex="atlas", normals="smooth", charts=4, materials=3), tmp_path), True, True)
    t = {k: _t(a[k]) for k in ("pos", "uv", "nrm")}
    i = {k: _t(a[k].astype(np.int32).reshape(-1, 3)) for k in ("pos_idx", "uv_idx", "nrm_idx")}
    mat = _t(a["materials"].view(np.int16))

    def make(t, i, mat):
        return cx.corner_mesh_from_tensors(t["pos"], i["pos_idx"], uv=t["uv"], uv_idx=i["uv_idx"], normals=t["nrm"], normal_idx=i["nrm_idx"], materials=mat)
    want = cx.write_hry(make(t, i, mat))
    for _ in range(3):
        t2, i2, m2 = {k: x * 1.0 for k, x in t.items()}, {k: x + 0 for k, x in i.items()}, mat + 0   # written by torch kernels right before the call
        assert cx.write_hry(make(t2, i2, m2)) == want
