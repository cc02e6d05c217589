"""Numbering maps of an encode on the GPU (include/harry_amd.h: hry_order_take; kernels: harry_amd/csrc/device/order.hip) through
Codec.write_hry(..., return_order=True): the device's maps against the restatement of tests/order_ref.py (pinned to the oracle by
tests/test_order_cpu.py), the source permuted by them against the product's own decode array for array, both profiles, general
bindings, rows moved through the maps, the composition with the ingest's weld, and the refusals.  Every comparison is exact.
(That an order handle's maps do not overlap and copy alike to host and device is checked with the other two handles in
tests/test_gpu_distortion.py, section 8.)"""
import ctypes as C

import numpy as np
import pytest

from harry_amd import _native as nat
from harry_amd import codec as hc
from harry_amd import meshgen as mg
from tests import order_ref as oref
from tests.test_order_cpu import MESHES, SCENES, load_scene, with_unreferenced

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DEV = torch.device("cuda", 0)
NO = nat.NO_ELEMENT
PROFILES = {"compat": hc.PROFILE_COMPAT, "chunked": hc.PROFILE_CHUNKED}
KINDS = ("vertex", "face", "corner")


@pytest.fixture(scope="module")
def cx():
    c = hc.Codec(0)
    yield c
    c.close()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def reference_maps(m: hc.Mesh, plain: bool, general: bool = False) -> dict:
    """the maps from a host walk of a copy of m (the walk repairs the copy's twins as the encode will m's)"""
    w = m.clone().host_walk(plain=plain)
    maps = oref.maps_from_walk(m, w["order_v"], w["order_f"])
    if general:
        maps.update(oref.record_maps_from_walk(m, w["order_v"], w["order_f"]))
    return maps


def device_maps(order: hc.Order) -> dict:
    return {name: order.numpy(name) for name in order.names}


def check_maps(m: hc.Mesh, got: dict, want: dict):
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name].dtype == np.uint32 and np.array_equal(got[name], want[name]), name
    unreferenced = m.nv - len(np.unique(m.org()))
    assert int((got["vertex"] == NO).sum()) == unreferenced
    for name in want:
        if name.endswith("_inv"):
            continue
        x, inv = got[name], got[name + "_inv"]
        coded = np.flatnonzero(x != NO)
        assert len(np.unique(x[coded])) == len(coded) and np.array_equal(inv[x[coded]], coded), name   # a bijection on what is coded
        assert int((inv != NO).sum()) == len(coded), name


def roundtrip(cx, m: hc.Mesh, profile: int, general: bool = False):
    """encode with the maps, decode; the maps on the host, checked against the reference; the decode"""
    want = reference_maps(m, plain=profile == hc.PROFILE_CHUNKED, general=general)
    data, order = cx.write_hry(m, profile=profile, return_order=True)
    try:
        got = device_maps(order)
    finally:
        order.close()
    check_maps(m, got, want)
    return data, got, cx.read_hry(data)


def check_ply_decode(m: hc.Mesh, maps: dict, dec: hc.Mesh):
    want = oref.permuted(m, maps, twin=m.twin())
    have = dict(oref.decoded_arrays(dec), twin=dec.twin())
    for key in ("face_offsets", "org", "twin", "vrec", "frec"):
        assert np.array_equal(have[key], want[key]), key


# ---- 1. the maps and the exact round trip, both profiles, lossless and -q12
@pytest.mark.parametrize("quant", ["lossless", "q12"])
@pytest.mark.parametrize("profile", sorted(PROFILES))
@pytest.mark.parametrize("name", sorted(MESHES))
def test_maps_and_exact_roundtrip(cx, name, profile, quant):
    m = hc.Mesh.from_ply(MESHES[name]().to_ply())
    if quant == "q12":
        cx.requant(m, [(1, -1, 12)])
    _, maps, dec = roundtrip(cx, m, PROFILES[profile])
    check_ply_decode(m, maps, dec)


# ---- 2. one numbering: compat and chunked give the same maps; the flag changes neither the container nor the twins
@pytest.mark.parametrize("name", ["multi_unreferenced", "soup", "torus_mixed"])
def test_profiles_agree_and_the_flag_changes_nothing(cx, name):
    ply = MESHES[name]().to_ply()
    per_profile = []
    for profile in (hc.PROFILE_COMPAT, hc.PROFILE_CHUNKED):
        a, b = hc.Mesh.from_ply(ply), hc.Mesh.from_ply(ply)
        plain = cx.write_hry(a, profile=profile)
        data, order = cx.write_hry(b, profile=profile, return_order=True)
        per_profile.append(device_maps(order))
        order.close()
        assert data == plain
        assert np.array_equal(a.twin(), b.twin())
    assert all(np.array_equal(per_profile[0][k], per_profile[1][k]) for k in per_profile[0])


def test_pipelined_chunked_encode_gives_the_same_maps(cx, monkeypatch):
    """components walked on several host threads with the device side beside the walk: the orders reach HBM run by run, inside the
    pipeline's batches, and order_f not at all when the mesh has no face records -- the maps' own upload"""
    monkeypatch.setenv("HRY_DEVICE_ANALYSIS_MIN_FACES", "1")
    monkeypatch.setenv("HRY_PARALLEL_MIN_FACES", "1")
    monkeypatch.setenv("HRY_HOST_THREADS", "6")
    monkeypatch.setenv("HRY_ENCODE_PIPELINE_BATCH", "40")
    for gen in (with_unreferenced(mg.with_nonmanifold(mg.multi_component(12, 9, 11, seed=8, polys="mixed"), 20, 10, seed=8)),
                mg.with_face_props(mg.multi_component(9, 9, 11, seed=9, polys="tri"))):
        m = hc.Mesh.from_ply(gen.to_ply())
        _, maps, dec = roundtrip(cx, m, hc.PROFILE_CHUNKED)
        check_ply_decode(m, maps, dec)


# ---- 3. general bindings: records through "list<l>", bindings through element and record maps, regions through "face"
@pytest.mark.parametrize("profile", sorted(PROFILES))
@pytest.mark.parametrize("name", sorted(SCENES))
def test_general_bindings(cx, name, profile, tmp_path):
    m = load_scene(SCENES[name](), tmp_path)
    assert m.general
    if name == "uv_normals_materials":
        assert m.nregions(0) == 3
        cx.requant(m, [(0, -1, 14), (2, -1, 11)])   # (quantised and lossless lists side by side)
    _, maps, dec = roundtrip(cx, m, PROFILES[profile], general=True)
    assert {f"list{l}" for l in range(m.nlists)} <= set(maps)
    want = oref.permuted_connectivity(m, maps, twin=m.twin())
    for key in ("face_offsets", "org", "twin"):
        assert np.array_equal(getattr(dec, key)(), want[key]), key
    oref.check_general_decode(m, dec, maps)


def test_ply_layout_has_no_list_names(cx):
    m = hc.Mesh.from_ply(MESHES["torus"]().to_ply())
    _, order = cx.write_hry(m, return_order=True)
    assert order.rows("list0") == 0 and order.rows("list1_inv") == 0 and order.data_ptr("list0") == 0
    assert (order.rows("vertex"), order.rows("face_inv"), order.rows("corner")) == (m.nv, m.nf, m.ne)
    with pytest.raises(hc.HryError) as e:
        order.numpy("list0")
    assert e.value.code == nat.E_ARG
    order.close()


# ---- 4. rows through the maps
@pytest.fixture(scope="module")
def unref(cx):
    """the mesh with unreferenced vertices, its maps on the host and their owner"""
    m = hc.Mesh.from_ply(MESHES["multi_unreferenced"]().to_ply())
    _, order = cx.write_hry(m, profile=hc.PROFILE_CHUNKED, return_order=True)
    yield m, order, device_maps(order)
    order.close()


def gathered(a: np.ndarray, idx: np.ndarray) -> np.ndarray:
    """numpy's fancy indexing with zero rows where the map says none"""
    out = np.zeros_like(a)
    ok = idx != NO
    out[ok] = a[idx[ok]]
    return out


ROWS = {
    "u8": (np.uint8, ()),
    "f32x3": (np.float32, (3,)),
    "i64x2": (np.int64, (2,)),
    "f16x5": (np.float16, (5,)),        # 10 bytes a row: the byte path
    "f32x257": (np.float32, (257,)),
    "f32x64": (np.float32, (64,)),      # 256 bytes a row: sixteen 16-byte units (i64x2 is one; f32x3 and f32x257 take the word path)
}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rows", sorted(ROWS))
def test_rows_through_the_maps(unref, kind, rows):
    m, order, maps = unref
    dtype, inner = ROWS[rows]
    n = len(maps[kind])
    rng = np.random.default_rng(11)
    a = rng.integers(1, 200, size=(n,) + inner).astype(dtype)   # (no zero anywhere: a zero row is a row the map left out)
    t = _t(a)
    dec = order.to_decoded(t, kind)
    assert dec.dtype == t.dtype and dec.shape == t.shape
    assert np.array_equal(dec.cpu().numpy(), gathered(a, maps[kind + "_inv"]))
    src = order.to_source(t, kind)
    assert np.array_equal(src.cpu().numpy(), gathered(a, maps[kind]))
    back = order.to_source(dec, kind).cpu().numpy()
    coded = maps[kind] != NO
    assert np.array_equal(back[coded], a[coded]) and not back[~coded].any()
    if kind == "vertex":
        assert (~coded).sum() == 3 and not dec.cpu().numpy()[maps["vertex_inv"] == NO].any()


@pytest.mark.parametrize("kind", KINDS)
def test_strided_rows(unref, kind):
    """a [:, 1:4] column view of [n, 6] float32 as source and as destination: the other columns of the destination stay"""
    m, order, maps = unref
    n = len(maps[kind])
    rng = np.random.default_rng(12)
    a = rng.integers(1, 200, size=(n, 6)).astype(np.float32)
    b = rng.integers(300, 400, size=(n, 6)).astype(np.float32)
    src, dst = _t(a), _t(b)
    got = order.to_decoded(src[:, 1:4], kind, out=dst[:, 1:4])
    assert got.data_ptr() == dst[:, 1:4].data_ptr()
    want = b.copy()
    want[:, 1:4] = gathered(a[:, 1:4], maps[kind + "_inv"])
    assert np.array_equal(dst.cpu().numpy(), want)
    assert np.array_equal(order.to_source(src[:, 1:4], kind).cpu().numpy(), gathered(a[:, 1:4], maps[kind]))
    # an odd byte offset: float16 columns 1..3 of [n, 4] start 2 bytes into 8-byte rows (the byte path with strides)
    h = rng.integers(1, 200, size=(n, 4)).astype(np.float16)
    assert np.array_equal(order.to_decoded(_t(h)[:, 1:4], kind).cpu().numpy(), gathered(h[:, 1:4], maps[kind + "_inv"]))


def test_tensor_is_int64_for_indexing(unref):
    m, order, maps = unref
    for name in ("vertex", "corner_inv"):
        t = order.tensor(name)
        assert t.dtype == torch.int64 and t.device == DEV
        want = maps[name].astype(np.int64)
        want[maps[name] == NO] = -1
        assert np.array_equal(t.cpu().numpy(), want)
    # torch's own gather agrees with to_decoded where the decoded row is real
    a = _t(np.arange(m.nv * 3, dtype=np.float32).reshape(m.nv, 3) + 1)
    inv = order.tensor("vertex_inv")
    real = inv >= 0
    assert torch.equal(order.to_decoded(a)[real], a.index_select(0, inv[real]))


# ---- 5. large meshes: every level of the scan of the decoded face offsets, many workgroups
# The offsets of a mixed-degree mesh are scanned by k_scan_sums / _top / _apply (twins.hip): blocks of 1024 faces, and one block that
# scans the block sums 1024 at a time -- its second round begins beyond 1024 * 1024 = 1 048 576 coded faces, the last level there is.
# mg.torus(840, 800, polys="mixed") is the smallest of this family's round sizes beyond it (1.6 faces a cell).  An all-triangle mesh
# needs no scan; it only has to span many workgroups.
def test_large_all_triangle_mesh(cx):
    m = hc.Mesh.from_ply(mg.torus(300, 200).to_ply())
    _, maps, dec = roundtrip(cx, m, hc.PROFILE_CHUNKED)
    check_ply_decode(m, maps, dec)


def test_large_mixed_mesh_crosses_every_scan_level(cx):
    m = hc.Mesh.from_ply(mg.torus(840, 800, polys="mixed").to_ply())
    assert m.nf > 1024 * 1024
    _, maps, dec = roundtrip(cx, m, hc.PROFILE_CHUNKED)
    check_ply_decode(m, maps, dec)


# ---- 6. composition with the ingest's weld
def test_composes_with_the_ingests_weld(cx):
    g = mg.soup()
    corners = g.verts[g.indices]                      # a triangle soup: one row per corner, equal rows where corners share a vertex
    xyz = np.stack([corners[k] for k in "xyz"], axis=1)
    idx = np.arange(len(corners), dtype=np.int32).reshape(-1, 3)
    m, remap = cx.mesh_from_tensors(_t(idx), [("x y z", _t(xyz))], weld=True, return_remap=True)
    assert m.nv < len(corners)
    data, order = cx.write_hry(m, profile=hc.PROFILE_CHUNKED, return_order=True)
    dec = cx.read_hry(data)
    to = order.tensor("vertex")[remap.long()]          # the decoded vertex of every input row
    assert int(to.min()) >= 0
    got = dec.list_data(1)[to.cpu().numpy()]
    assert np.array_equal(got, np.ascontiguousarray(xyz).view(np.uint8).reshape(len(corners), 12))
    order.close()


# ---- 7. refusals; the context stays usable, the handle outlives what the context does
def _refused(code, fn, *args, **kw):
    with pytest.raises(hc.HryError) as e:
        fn(*args, **kw)
    assert e.value.code == code, e.value
    return e.value


def _usable(cx, m):
    data, order = cx.write_hry(m.clone(), return_order=True)
    assert order.rows("vertex") == m.nv and len(data)
    order.close()


def test_take_refusals(cx):
    m = hc.Mesh.from_ply(MESHES["torus"]().to_ply())
    cx.write_hry(m)
    e = _refused(nat.E_ARG, cx.take_order, m)                     # no flag
    assert "HRY_FLAG_ORDER" in e.msg
    _usable(cx, m)
    data = cx.write_hry(m, flags=hc.FLAG_ORDER)
    cx.read_hry(data)
    _refused(nat.E_ARG, cx.take_order, m)                         # another call on the context in between
    _usable(cx, m)
    cx.write_hry(m, flags=hc.FLAG_ORDER)
    other = hc.Mesh.from_ply(MESHES["torus"]().to_ply())
    _refused(nat.E_ARG, cx.take_order, other)                     # another mesh
    order = cx.take_order(m)
    _refused(nat.E_ARG, cx.take_order, m)                         # a second take
    assert order.rows("face") == m.nf
    order.close()
    _usable(cx, m)


def test_sharding_refuses_the_flag(cx):
    m = hc.Mesh.from_ply(MESHES["multi"]().to_ply())
    shard = hc.ShardPlan(m, 2).extract(m, 0)
    assert len(shard.runs())
    _refused(nat.E_UNSUPPORTED, cx.write_hry, shard, profile=hc.PROFILE_CHUNKED, return_order=True)
    assert len(cx.write_hry(shard, profile=hc.PROFILE_CHUNKED))   # (without the flag the shard codes, on the same context)
    mc = hc.MultiCodec([0, 0])
    try:
        _refused(nat.E_UNSUPPORTED, mc.write_hry, m, return_order=True)
        assert len(mc.write_hry(m))
    finally:
        mc.close()
    _usable(cx, m)


def test_apply_refusals(cx, unref):
    m, order, maps = unref
    L = nat.load()
    n = m.nv
    src, dst = torch.ones(n, 4, dtype=torch.float32, device=DEV), torch.zeros(n, 4, dtype=torch.float32, device=DEV)
    host = np.zeros((n, 4), np.float32)
    torch.cuda.synchronize()

    def apply(kind=b"vertex", direction=0, s=None, ss=16, d=None, ds=16, row=16, rows=n):
        return L.hry_order_apply(cx.h, order.h, kind, direction, src.data_ptr() if s is None else s, ss, dst.data_ptr() if d is None else d, ds, row, rows)

    assert apply() == nat.OK
    cases = {
        "src stride below row_bytes": dict(ss=12), "dst stride below row_bytes": dict(ds=8), "row_bytes 0": dict(row=0, ss=0, ds=0),
        "null src": dict(s=C.c_void_p(None)), "null dst": dict(d=C.c_void_p(None)), "host src": dict(s=host.ctypes.data), "host dst": dict(d=host.ctypes.data),
        "overlap": dict(d=src.data_ptr() + 16 * (n // 2)), "same buffer": dict(d=src.data_ptr()),
        "interleaved columns": dict(s=src.data_ptr(), d=src.data_ptr() + 8, ss=16, ds=16, row=8),
        "unknown kind": dict(kind=b"edge"), "inverse as kind": dict(kind=b"vertex_inv"), "absent list": dict(kind=b"list0"),
        "unknown direction": dict(direction=2), "wrong rows": dict(rows=n - 1),
    }
    for what, kw in cases.items():
        assert apply(**kw) == nat.E_ARG, what
        assert L.hry_last_error(), what
        _usable(cx, m)
    assert apply(kind=None) == nat.E_ARG
    assert torch.equal(dst[maps["vertex_inv"] != NO], src[maps["vertex_inv"] != NO])   # (the one good call's rows are still there)
    # the Python surface refuses what it can see before the library does
    _refused(nat.E_ARG, order.to_decoded, torch.ones(n, 4), "vertex")                        # a host tensor
    _refused(nat.E_ARG, order.to_decoded, src[:, ::2], "vertex")                              # inner dimension not contiguous
    _refused(nat.E_ARG, order.to_decoded, src[: n - 1], "vertex")                            # wrong row count
    _refused(nat.E_ARG, order.to_decoded, src, "face")


def test_handle_outlives_the_contexts_work(cx):
    m = hc.Mesh.from_ply(MESHES["torus_mixed"]().to_ply())
    data, order = cx.write_hry(m, profile=hc.PROFILE_CHUNKED, return_order=True)
    before = device_maps(order)
    other = hc.Codec(0)
    other.write_hry(m.clone())
    other.close()
    big = hc.Mesh.from_ply(mg.torus(90, 80, normals=True).to_ply())   # (larger than m: the context's buffers grow, and are reused)
    for profile in (hc.PROFILE_COMPAT, hc.PROFILE_CHUNKED):
        d2, o2 = cx.write_hry(big, profile=profile, return_order=True)
        o2.close()
        cx.read_hry(d2)
    after = device_maps(order)
    assert all(np.array_equal(before[k], after[k]) for k in before)
    a = _t(np.arange(m.nf, dtype=np.int32) + 1)
    assert np.array_equal(order.to_decoded(a, "face").cpu().numpy(), gathered(np.arange(m.nf, dtype=np.int32) + 1, before["face_inv"]))
    order.close()
    order.close()   # (closing twice is harmless)
