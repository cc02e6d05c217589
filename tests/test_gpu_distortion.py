"""Per-component error of a decode on the GPU (include/harry_amd.h: hry_distortion_build; kernels: harry_amd/csrc/device/distortion.hip)
through Codec.distortion, against the restatement of tests/distortion_ref.py (pinned by tests/test_distortion_cpu.py).  The values the
restatement compares come from Codec.requant(clear=True) -- k_requant, pinned to the reference's goldens -- read through
Mesh.component; the maps come from the Order handle (pinned by tests/test_gpu_order.py).  Every comparison is exact, except sum_sq and
sum_sq_dist: rows * 2^-52 relative to math.fsum (tests/distortion_ref.py: sum_tolerance -- derived, not measured).

Not covered here: a quantised list whose bounds were never set (HRY_E_ARG, the check hry_render_build shares).  No constructor,
reader or decode of the public interface returns such a mesh: hry_requant computes the bounds it needs, a .hry header carries them,
and hry_list_set_bounds refuses a quantised list.  Lossless `double` components are outside the codec's subset (hry_encode refuses
them), so mg.doubles round-trips at -q12 only."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from harry_amd import _native as nat
from harry_amd import cli
from harry_amd import codec as hc
from harry_amd import meshgen as mg
from tests import distortion_ref as dref
from tests import util
from tests.test_order_cpu import MESHES, SCENES, load_scene

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
NO = nat.NO_ELEMENT
PROFILES = {"compat": hc.PROFILE_COMPAT, "chunked": hc.PROFILE_CHUNKED}
EXACT = ("max_abs", "a_min", "a_max", "compared", "skipped", "nonfinite", "changed", "argmax")


@pytest.fixture(scope="module")
def cx():
    c = hc.Codec(0)
    yield c
    c.close()


def cleared(cx, m: hc.Mesh) -> hc.Mesh:
    c = m.clone()
    cx.requant(c, [], clear=True)
    return c


def compared_lists(m: hc.Mesh):
    return [l for l in range(m.nlists) if len(m.list_fmt(l)) and m.list_target(l) <= 2 and (m.general or l < 2)]


def list_bytes(m: hc.Mesh) -> int:
    return sum(m.list_count(l) * m.list_stride(l) for l in compared_lists(m))


def reference(cx, a: hc.Mesh, b: hc.Mesh, maps: dict, pos_list) -> dict:
    """the restatement per compared list (call it after the builds under test: requant is a call on the context)"""
    ca, cb = cleared(cx, a), cleared(cx, b)
    return {l: dref.compare(dref.values(ca, l), dref.values(cb, l), maps.get(l), pos=0 if l == pos_list else None) for l in compared_lists(a)}


def close_sum(got: float, want: float, rows: int) -> bool:
    return abs(got - want) <= dref.sum_tolerance(max(rows, 1)) * want


def check(d: hc.Distortion, a: hc.Mesh, ref: dict, pos_list, rows: bool = True):
    for l, r in ref.items():
        n = a.list_count(l)
        for c, want in enumerate(r["comp"]):
            got = d.component(l, c)
            print(f"list {l} comp {c}: got {got}\n               want {want}")
            for k in EXACT:
                assert got[k] == want[k], (l, c, k, got[k], want[k])
            assert close_sum(got["sum_sq"], want["sum_sq"], n), (l, c, got["sum_sq"], want["sum_sq"])
            assert got["rms"] == (math.sqrt(got["sum_sq"] / got["compared"]) if got["compared"] else 0.0)
        if rows:
            err = d.numpy(f"error{l}")
            assert err.dtype == np.float32 and np.array_equal(err.view(np.uint32), r["rows"].view(np.uint32)), f"error{l}"
        else:
            assert d.rows(f"error{l}") == 0 and d.data_ptr(f"error{l}") == 0
    p = d.position()
    if pos_list is None:
        assert (p["list"], p["compared"], p["max_dist"], p["sum_sq_dist"], p["psnr"]) == (-1, 0, 0.0, 0.0, math.inf)
        return
    want = ref[pos_list]["pos"]
    print(f"position: got {p}\n          want {want}")
    assert p["list"] == pos_list and nat.load().hry_distortion_position_component(d.h) == 0
    for k in ("max_dist", "compared", "argmax"):
        assert p[k] == want[k], (k, p[k], want[k])
    assert close_sum(p["sum_sq_dist"], want["sum_sq_dist"], a.list_count(pos_list))
    comps = ref[pos_list]["comp"][:3]
    diagonal = math.sqrt(sum(x * x for x in [c["a_max"] - c["a_min"] for c in comps]))
    assert p["diagonal"] == diagonal and p["rms"] == (math.sqrt(p["sum_sq_dist"] / p["compared"]) if p["compared"] else 0.0)
    assert p["psnr"] == (20.0 * math.log10(diagonal / p["rms"]) if p["rms"] > 0 else math.inf)
    with pytest.raises(hc.HryError):
        d.component(len(ref) + 40, 0)
    with pytest.raises(hc.HryError):
        d.component(pos_list, 99)


# ---- 1. round trips through the codec, both profiles
ROUNDTRIP = dict(MESHES, doubles=lambda: mg.doubles(mg.torus(24, 16)), colors=lambda: mg.with_colors(mg.torus(12, 14)))
QUANTS = {"lossless": [], "q12": [(1, -1, 12)], "q8": [(1, -1, 8)]}
COLORS_Q12 = [(1, 0, 12), (1, 1, 12), (1, 2, 12)]   # (hry_requant refuses 12 bits for a uchar: the colours stay lossless there)
CASES = [(n, q) for n in sorted(ROUNDTRIP) for q in ("lossless", "q12") if (n, q) != ("doubles", "lossless")] + [("colors", "q8")]


@pytest.mark.parametrize("profile", sorted(PROFILES))
@pytest.mark.parametrize("name,quant", CASES, ids=[f"{n}-{q}" for n, q in CASES])
def test_roundtrip(cx, name, quant, profile):
    src = hc.Mesh.from_ply(ROUNDTRIP[name]().to_ply())
    enc = src.clone()
    quants = COLORS_Q12 if (name, quant) == ("colors", "q12") else QUANTS[quant]
    if quants:
        cx.requant(enc, quants)
    data, order = cx.write_hry(enc, profile=PROFILES[profile], return_order=True)
    dec = cx.read_hry(data)
    d = cx.distortion(src.clone(), dec, order, rows=True)
    maps = {1: order.numpy("vertex"), 0: order.numpy("face")}
    order.close()
    ref = reference(cx, src, dec, maps, 1)
    check(d, src, ref, 1)
    if quant == "lossless":
        for l, r in ref.items():
            for c in range(len(r["comp"])):
                got = d.component(l, c)
                assert (got["max_abs"], got["sum_sq"], got["changed"]) == (0.0, 0.0, 0)
        assert d.position()["psnr"] == math.inf and not d.numpy("error1").any()
    else:
        assert d.component(1, 0)["changed"] > 0 and d.position()["max_dist"] > 0
    if name == "multi_unreferenced":
        assert d.component(1, 0)["skipped"] == 3 == src.nv - len(np.unique(src.org()))
    if (name, quant) == ("colors", "q8"):
        # integers are truncated twice (quant.h:103-107), 8 bits over an extent of at most 255: the value comes back itself or one below
        for c in (3, 4, 5):
            got = d.component(1, c)
            assert got["max_abs"] == 1.0 and got["sum_sq"] == got["changed"]
    d.close()
    d.close()   # (closing twice is harmless)


# ---- 2. general bindings: records paired through "list<l>"
@pytest.mark.parametrize("name", sorted(SCENES))
def test_general_bindings(cx, name, tmp_path):
    src = load_scene(SCENES[name](), tmp_path)
    assert src.general
    enc = src.clone()
    cx.requant(enc, [(0, -1, 14), (1, -1, 10)])
    data, order = cx.write_hry(enc, profile=hc.PROFILE_CHUNKED, return_order=True)
    dec = cx.read_hry(data)
    d = cx.distortion(src, dec, order, rows=True)
    maps = {l: order.numpy(f"list{l}") for l in range(src.nlists)}
    order.close()
    assert src.list_target(0) == 1
    ref = reference(cx, src, dec, maps, 0)
    assert sorted(ref) == compared_lists(src) and len(ref) >= 2
    check(d, src, ref, 0)
    for l in ref:
        assert d.component(l, 0)["skipped"] == int((maps[l] == NO).sum())   # records that nothing names are never coded
    assert d.component(0, 0)["changed"] > 0 and d.component(1, 0)["changed"] > 0
    d.close()


# ---- 3. the identity with planted errors, no codec: more than one block, a tail, the second stage
def test_identity_with_planted_errors(cx):
    g = mg.grid(363, 362)
    nv = g.nv
    assert nv >= 2 ** 17 + 5 and nv % 1024 and nv % 256
    va, vb = g.verts.copy(), g.verts.copy()
    mid, nan_row, inf_row = nv // 2 + 3, nv // 3, 2 * nv // 3 + 1
    for rows, x, y in (((0, nv - 1), 1.0, 1.5), ((mid,), 3.0, 3.25)):   # the same largest error in the first and the last row
        for r in rows:
            va["x"][r], vb["x"][r] = x, y
    va["y"][nan_row] = vb["y"][nan_row] = np.float32(math.nan)          # the same bits on both sides: non-finite, not changed
    vb["z"][inf_row] = np.float32(math.inf)                             # on one side only: non-finite and changed
    a, b = hc.Mesh.from_arrays(va, g.degrees, g.indices), hc.Mesh.from_arrays(vb, g.degrees, g.indices)
    d = cx.distortion(a, b, rows=True)
    cx_, cy, cz = (d.component(1, c) for c in range(3))
    assert (cx_["max_abs"], cx_["argmax"], cx_["sum_sq"], cx_["compared"], cx_["skipped"], cx_["nonfinite"], cx_["changed"]) == (0.5, 0, 0.5625, nv, 0, 0, 3)
    assert (cx_["a_min"], cx_["a_max"]) == (float(va["x"].min()), float(va["x"].max()))
    assert (cy["max_abs"], cy["argmax"], cy["sum_sq"], cy["compared"], cy["nonfinite"], cy["changed"]) == (0.0, 0, 0.0, nv - 1, 1, 0)
    assert (cz["max_abs"], cz["argmax"], cz["sum_sq"], cz["compared"], cz["nonfinite"], cz["changed"]) == (0.0, 0, 0.0, nv - 1, 1, 1)
    p = d.position()
    assert (p["list"], p["max_dist"], p["argmax"], p["sum_sq_dist"], p["compared"]) == (1, 0.5, 0, 0.5625, nv - 2)
    want = np.zeros(nv, np.float32)
    want[[0, nv - 1, mid]] = [0.5, 0.5, 0.25]
    assert np.array_equal(d.numpy("error1"), want)
    t = d.tensor("error1")
    assert t.dtype == torch.float32 and t.device == torch.device("cuda", 0) and np.array_equal(t.cpu().numpy(), want)
    assert d.rows("error0") == 0   # (the face list has no components: not compared)
    with pytest.raises(hc.HryError):
        d.component(0, 0)
    assert d.stat()["uploaded_bytes"] == 2 * nv * 12 and d.stat()["device_ms"] > 0
    check(d, a, reference(cx, a, b, {}, 1), 1)
    # the largest error only in the last row, and a larger one in the tail's last lane
    vb["x"][0] = va["x"][0]
    vb["x"][nv - 1] = 2.0
    b2 = hc.Mesh.from_arrays(vb, g.degrees, g.indices)
    d2 = cx.distortion(a, b2)
    assert (d2.component(1, 0)["max_abs"], d2.component(1, 0)["argmax"], d2.component(1, 0)["changed"]) == (1.0, nv - 1, 2)
    assert d2.rows("error1") == 0
    d.close(), d2.close()


# ---- 4. thirty-two components of mixed types: strides, offsets, the 64-bit conversions
def test_thirty_two_mixed_components(cx):
    g = mg.grid(40, 39)
    nv = g.nv
    kinds = ["<f4", "<f8", "<i4", "<i2", "u1", "<u8"]
    names = ["x", "y", "z"] + [f"p{k}" for k in range(3, 32)]
    types = ["<f4", "<f4", "<f4"] + [kinds[k % 6] for k in range(3, 32)]
    rng = np.random.default_rng(5)
    va = np.zeros(nv, np.dtype(list(zip(names, types))))
    for n, t in zip(names, types):
        if n in "xyz":
            va[n] = g.verts[n]
        elif t == "<u8":
            va[n] = rng.integers(0, 2 ** 64, nv, dtype=np.uint64)   # beyond 2^53: the conversion to double rounds
        elif t[1] == "f":
            va[n] = rng.normal(0, 1e3, nv)
        else:
            info = np.iinfo(np.dtype(t))
            va[n] = rng.integers(info.min, int(info.max) + 1, nv, dtype=np.int64).astype(t)
    vb = va.copy()
    iw = types.index("<u8")
    last, wide = names[31], names[iw]
    assert types[31] == "<f8" and set(types) == set(kinds)
    vb[last][[7, nv - 2]] += 0.75
    va[wide][11], vb[wide][11] = 2 ** 60 + 1, 2 ** 60 + 1024          # (2^60 + 1 rounds to 2^60)
    va[wide][nv - 1], vb[wide][nv - 1] = 2 ** 63 + 2 ** 20, 2 ** 63    # above the signed range
    a, b = hc.Mesh.from_arrays(va, g.degrees, g.indices), hc.Mesh.from_arrays(vb, g.degrees, g.indices)
    assert len(a.list_fmt(1)) == 32
    d = cx.distortion(a, b, rows=True)
    w = d.component(1, iw)
    assert (w["max_abs"], w["argmax"], w["changed"], w["compared"]) == (float(2 ** 20), nv - 1, 2, nv) and w["sum_sq"] == float(2 ** 40) + float(2 ** 20)
    e = d.component(1, 31)
    assert (e["argmax"], e["changed"], e["nonfinite"]) == (7, 2, 0) and abs(e["max_abs"] - 0.75) < 1e-9
    check(d, a, reference(cx, a, b, {}, 1), 1)
    d.close()


# ---- 5. determinism and residency
def _snapshot(d: hc.Distortion, m: hc.Mesh) -> tuple:
    comps = tuple(tuple(sorted(d.component(l, c).items())) for l in compared_lists(m) for c in range(len(m.list_fmt(l))))
    return comps, tuple(sorted(d.position().items())), tuple(d.numpy(f"error{l}").tobytes() for l in compared_lists(m))


def test_determinism_and_residency(cx):
    src = hc.Mesh.from_ply(mg.with_face_props(mg.torus(40, 37, normals=True)).to_ply())
    enc = src.clone()
    cx.requant(enc, [(1, -1, 12)])
    data, order = cx.write_hry(enc, profile=hc.PROFILE_CHUNKED, return_order=True)
    dec = cx.read_hry(data)
    d1 = cx.distortion(src, dec, order, rows=True)
    assert d1.stat()["uploaded_bytes"] == list_bytes(src)        # a from the host, nothing of b: the decode left it in HBM
    d2 = cx.distortion(src, dec, order, rows=True)
    assert d2.stat()["uploaded_bytes"] == list_bytes(src)        # (the build does not disturb what it reads)
    snap = _snapshot(d1, src)
    assert _snapshot(d2, src) == snap
    copy = dec.clone()                                           # not resident: b goes up too, with the same results
    d3 = cx.distortion(src, copy, order, rows=True)
    assert d3.stat()["uploaded_bytes"] == list_bytes(src) + list_bytes(copy) > d1.stat()["uploaded_bytes"]
    assert _snapshot(d3, src) == snap
    assert (order.numpy("vertex") != NO).all() and order.rows("face") == src.nf      # the order is still a handle of its own
    got = cx.render(dec)                                                               # ... and the decode is still where it was
    assert cx.render_stat()["uploaded_bytes"] == 0 and got["list1"].shape == (dec.nv, 6)
    # a resident on the context (an upload), b from the host
    cx.upload(src)
    assert cx.resident(src)
    d4 = cx.distortion(src, copy, order, rows=True)
    assert d4.stat()["uploaded_bytes"] == list_bytes(copy)
    assert _snapshot(d4, src) == snap and cx.resident(src)
    assert snap[0][0] != snap[0][1] and d1.component(1, 0)["changed"] > 0
    for d in (d1, d2, d3, d4):
        d.close()
    order.close()


# ---- 6. refusals; each leaves the context usable
def _refused(code, fn, *args, **kw):
    with pytest.raises(hc.HryError) as e:
        fn(*args, **kw)
    assert e.value.code == code, e.value
    return e.value


def test_refusals(cx, tmp_path):
    ply = MESHES["torus"]().to_ply()
    m = hc.Mesh.from_ply(ply)
    small = hc.Mesh.from_ply(mg.torus(12, 10).to_ply())
    data, order = cx.write_hry(m.clone(), return_order=True)
    dec = cx.read_hry(data)
    _, small_order = cx.write_hry(small.clone(), return_order=True)

    def usable():
        d = cx.distortion(m, dec, order)
        assert d.component(1, 0)["compared"] == m.nv and d.component(1, 0)["max_abs"] == 0.0
        d.close()

    usable()
    scene = load_scene(SCENES["uv_normals_materials"](), tmp_path)
    assert scene.nlists != m.nlists
    cases = {
        "different list counts": (m, scene, None),
        "different component types": (m, hc.Mesh.from_ply(mg.doubles(MESHES["torus"]()).to_ply()), None),
        "unequal counts without an order": (m, small, None),
        "an order of another mesh": (m, dec, small_order),
        "a map entry at or above b's count": (m, small, order),
    }
    for what, (a, b, o) in cases.items():
        e = _refused(nat.E_ARG, cx.distortion, a, b, o, rows=True)
        if what.startswith(("an order", "a map entry")):
            assert "order does not fit the meshes" in e.msg, what
        usable()
    multi = hc.Mesh.from_ply(MESHES["multi"]().to_ply())
    shard = hc.ShardPlan(multi, 2).extract(multi, 0)
    part = cx.read_hry(cx.write_hry(shard, profile=hc.PROFILE_CHUNKED), partial=True)
    assert part.partial
    _refused(nat.E_ARG, cx.distortion, multi, part)
    _refused(nat.E_ARG, cx.distortion, part, multi)
    usable()
    h = C.c_void_p(1)
    L = nat.load()
    assert L.hry_distortion_build(cx.h, m.h, dec.h, order.h, 2, C.byref(h)) == nat.E_ARG and not h.value   # an unknown flag; *out is NULL
    assert b"flag" in L.hry_last_error()
    assert L.hry_distortion_build(cx.h, m.h, None, None, 0, C.byref(h)) == nat.E_ARG and not h.value
    usable()
    order.close()
    small_order.close()


# ---- 7. the command line
def test_cli_report(cx, tmp_path):
    gen = mg.torus(24, 16, normals=True)
    src, out, plain = tmp_path / "in.ply", tmp_path / "out.hry", tmp_path / "plain.hry"
    src.write_bytes(gen.to_ply())
    r = subprocess.run([cli.HARRY, str(src), str(out), "-l1", "-q12", "--report"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r0 = subprocess.run([cli.HARRY, str(src), str(plain), "-l1", "-q12"], capture_output=True, text=True, timeout=300)
    assert r0.returncode == 0 and "Distortion:" not in r0.stdout
    assert out.read_bytes() == plain.read_bytes()
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("Distortion:")]
    a = hc.Mesh.from_ply(src.read_bytes())
    q = a.clone()
    cx.requant(q, [(1, -1, 12)])
    d = cx.distortion(a, q)
    assert len(lines) == 6 == len(a.list_fmt(1))
    for c, w in enumerate(lines):
        assert w[1:8:2] == ["list", "attr", "bits", "max"] and w[9] == "rms" and w[11] == "changed"
        want = d.component(1, c)
        bits = q.list_fmt(1)[c][1]
        assert (int(w[2]), int(w[4]), int(w[6]), int(w[12])) == (1, c, bits, want["changed"]) and bits == 12
        for got, ref in ((float(w[8]), want["max_abs"]), (float(w[10]), want["rms"])):
            assert abs(got - ref) <= 1e-8 * abs(ref), (c, got, ref)
    d.close()


# ---- 8. the buffers of a render, an order and a distortion handle: found by name in one allocation, owned by the handle
GOLD = os.path.join(util.ROOT, "tests", "golden")
ELEMENT_BYTES = {0: 4, 4: 4, 6: 2}   # HRY_FLOAT, HRY_UINT, HRY_USHORT
TORCH_OF = {0: torch.float32, 4: torch.int32, 6: torch.int16}


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def _one_triangle():
    v = np.zeros(3, np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4")]))
    v["x"], v["y"] = [0, 1, 0], [0, 0, 1]
    return hc.Mesh.from_arrays(v, np.array([3], np.uint8), np.array([0, 1, 2], np.uint32))


HANDLE_MESHES = {
    "one_triangle": _one_triangle,
    "torus_mixed": lambda: hc.Mesh.from_ply(_read(os.path.join(GOLD, "torus_mixed.ply"))),                           # mixed degrees, PLY layout
    "smooth_obj": lambda: hc.Mesh.from_obj(_read(os.path.join(GOLD, "obj", "smooth.obj")), os.path.join(GOLD, "obj")),   # corner lists: the unweld, "list<l>" maps
}


class Handles:
    """of one mesh on cx: its encode's order handle, a render handle of the decode with both normals flags and a distortion handle
    with HRY_DISTORTION_ROWS, each read through the C interface alone"""

    def __init__(self, cx, src: hc.Mesh):
        L = nat.load()
        self.cx, self.src = cx, src
        data, self.order = cx.write_hry(src.clone(), profile=hc.PROFILE_CHUNKED, return_order=True)
        self.dec = cx.read_hry(data)
        self.dist = cx.distortion(src, self.dec, self.order, rows=True)
        self.render = C.c_void_p()
        nat.check(L.hry_render_build_ex(cx.h, self.dec.h, hc.Codec.RENDER_VERTEX_NORMALS | hc.Codec.RENDER_FACE_NORMALS, C.byref(self.render)))
        lists = tuple(f"list{l}" for l in range(src.nlists))
        self.h = {"render": self.render, "order": self.order.h, "distortion": self.dist.h}
        self.names = {"render": hc.Codec.RENDER_FIXED + lists + hc.Codec.RENDER_NORMALS,
                      "order": tuple(n + sfx for n in hc.Order.KINDS + lists for sfx in ("", "_inv")),
                      "distortion": tuple(f"error{l}" for l in range(src.nlists))}

    def close(self):
        nat.load().hry_render_free(self.render)
        self.dist.close()
        self.order.close()

    def get(self, kind: str, name: str) -> tuple:
        """(device address, rows, width, component type) of a buffer; rows 0: the handle has none of that name"""
        L = nat.load()
        dev, rows, width, typ = C.c_void_p(), C.c_uint64(), C.c_int(1), C.c_int(4 if kind == "order" else 0)
        if kind == "render":
            nat.check(L.hry_render_get(self.h[kind], name.encode(), C.byref(dev), C.byref(rows), C.byref(width), C.byref(typ)))
        else:
            nat.check(getattr(L, f"hry_{kind}_get")(self.h[kind], name.encode(), C.byref(dev), C.byref(rows)))
        return dev.value or 0, rows.value, width.value, typ.value

    def copy(self, kind: str, name: str, dst, on_device: bool) -> int:
        return getattr(nat.load(), f"hry_{kind}_copy")(self.cx.h, self.h[kind], name.encode(), dst, int(on_device))

    def present(self, kind: str) -> list:
        return [n for n in self.names[kind] if self.get(kind, n)[1]]

    def host_bytes(self, kind: str, name: str) -> bytes:
        _, rows, width, typ = self.get(kind, name)
        a = np.empty(rows * width * ELEMENT_BYTES[typ], np.uint8)
        assert self.copy(kind, name, a.ctypes.data, False) == nat.OK, (kind, name)
        return a.tobytes()

    def results(self) -> dict:
        """every buffer of the three handles as host bytes and what else a build computes: the same from every build of one mesh"""
        L = nat.load()
        out = {(kind, n): self.host_bytes(kind, n) for kind in self.h for n in self.present(kind)}
        out["render counts"] = (L.hry_render_nverts(self.render), L.hry_render_ntris(self.render))
        out["distortion"] = _snapshot(self.dist, self.src)[:2]
        return out

    def snapshot(self) -> dict:
        """... and the statistics, which hold the build's own times"""
        d, up = C.c_double(), C.c_uint64()
        nat.check(nat.load().hry_render_stat(self.render, C.byref(d), C.byref(up)))
        return dict(self.results(), render_stat=(d.value, up.value), distortion_stat=tuple(sorted(self.dist.stat().items())))


@pytest.mark.parametrize("name", sorted(HANDLE_MESHES))
def test_buffers_of_a_handle_are_disjoint_and_copy_both_ways(cx, name):
    src = HANDLE_MESHES[name]()
    H = Handles(cx, src)
    L = nat.load()
    dev = torch.device("cuda", 0)

    def usable():   # the context builds good results again: those of the first build
        again = Handles(cx, src)
        try:
            assert again.results() == first
        finally:
            again.close()

    try:
        first = H.results()
        assert H.present("render")[:3] == ["indices", "tri_face", "vertex_source"] and {"normals", "face_normals"} <= set(H.present("render"))
        assert {"vertex", "vertex_inv", "face", "face_inv", "corner", "corner_inv"} <= set(H.present("order"))
        assert H.present("distortion") == [f"error{l}" for l in compared_lists(src)] and H.present("distortion")
        if src.general:
            assert "corner_source" in H.present("render") and "face_region" in H.present("render") and "list1_inv" in H.present("order")
        for kind in H.h:
            spans = []
            for n in H.present(kind):
                addr, rows, width, typ = H.get(kind, n)
                assert addr != 0 and width >= 1, (kind, n)
                spans.append((addr, addr + rows * width * ELEMENT_BYTES[typ], n))
                torch.cuda.current_stream(dev).synchronize()
                t = torch.empty((rows * width,), dtype=TORCH_OF[typ], device=dev)
                assert H.copy(kind, n, t.data_ptr(), True) == nat.OK, (kind, n)
                assert t.cpu().numpy().tobytes() == first[(kind, n)], (kind, n)   # device to device, then down through torch
            spans.sort()
            for (_, end, n0), (start, _, n1) in zip(spans, spans[1:]):
                assert end <= start, (kind, n0, n1, [(hex(a), e - a, n) for a, e, n in spans])
            # an absent name, then a NULL destination for a buffer that has rows
            host = np.zeros(16, np.uint8)
            assert H.get(kind, "no_such_buffer")[:2] == (0, 0)
            assert H.copy(kind, "no_such_buffer", host.ctypes.data, False) == nat.E_ARG and L.hry_last_error()
            usable()
            for on_device in (False, True):
                assert H.copy(kind, H.present(kind)[0], None, on_device) == nat.E_ARG and L.hry_last_error()
            usable()
        assert H.results() == first
    finally:
        H.close()


def test_render_and_distortion_handles_outlive_the_contexts_work(cx, tmp_path):
    """(tests/test_gpu_order.py: test_handle_outlives_the_contexts_work, for the other two handles)"""
    H = Handles(cx, HANDLE_MESHES["smooth_obj"]())
    P = Handles(cx, HANDLE_MESHES["torus_mixed"]())
    try:
        before = H.snapshot(), P.snapshot()
        big = hc.Mesh.from_ply(mg.torus(90, 80, polys="mixed", normals=True).to_ply())   # (larger than either: the context's buffers grow, and are reused)
        for profile in (hc.PROFILE_COMPAT, hc.PROFILE_CHUNKED):
            data, order = cx.write_hry(big.clone(), profile=profile, return_order=True)
            dec = cx.read_hry(data)
            assert len(cx.render_numpy(dec, normals="area", face_normals=True)["normals"]) == big.nv
            cx.distortion(big, dec, order, rows=True).close()
            order.close()
        sc = load_scene(SCENES["uv_normals_materials"](), tmp_path)
        assert "corner_source" in cx.render_numpy(cx.read_hry(cx.write_hry(sc, profile=hc.PROFILE_CHUNKED)))
        assert (H.snapshot(), P.snapshot()) == before
    finally:
        H.close()
        P.close()
