"""Render-ready device buffers (include/harry_amd.h: hry_render_build; kernels: harry_amd/csrc/device/render.hip) against the
numpy restatement of tests/render_ref.py: fan triangulation, float columns after the reference's `-c` dequantisation (pinned to the
reference's own dequantised goldens), the unweld of general bindings, residency after a decode, and the torch interface.
(That a render handle's buffers do not overlap, copy alike to host and device and outlive the context's later work is checked
with the other two handles in tests/test_gpu_distortion.py, section 8.)"""
import ctypes as C
import json
import os

import numpy as np
import pytest

from harry_amd import _native as nat
from harry_amd import codec as hc
from harry_amd import meshgen as mg
from harry_amd import objgen as og
from oracle import oracle_py as op
from tests import render_ref as rr
from tests import util

pytestmark = pytest.mark.gpu

GOLD = os.path.join(util.ROOT, "tests", "golden")
OBJ = os.path.join(GOLD, "obj")


def _read(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def cx():
    c = hc.Codec(0)
    yield c
    c.close()


def rows_to_records(mesh, l, vsrc, csrc):
    """record of list l named by every output row (NONE: unbound)"""
    t = mesh.list_target(l)
    if not mesh.general:
        return np.arange(mesh.nf if t == 0 else mesh.nv, dtype=np.int64)
    if t == 0:
        elem, owner_reg, which, kind = np.arange(mesh.nf), mesh.regions_of(0), 0, 0
        reg = owner_reg
    elif t == 1:
        elem, reg, which, kind = vsrc.astype(np.int64), mesh.regions_of(1)[vsrc], 1, 1
    else:
        if csrc is None:
            return np.full(len(vsrc), -1, np.int64)
        elem = csrc.astype(np.int64)
        eface = np.repeat(np.arange(mesh.nf), np.diff(mesh.face_offsets().astype(np.int64)))
        reg, which, kind = mesh.regions_of(0)[eface[elem]], 0, 2
    b = mesh.bindings(kind)
    out = np.full(len(elem), -1, np.int64)
    nreg = mesh.nregions(which)
    for r in range(nreg):
        lists = mesh.region_lists(kind, r)
        if l in lists:
            sel = reg == r
            out[sel] = b[elem[sel], lists.index(l)]
    return out


def expected(mesh, cleared):
    """the restatement of every buffer; `cleared`: the same mesh after hry_requant(clear) (its records give the values)"""
    cmap, vsrc, csrc = rr.vertex_map(mesh)
    idx, tri_face = rr.fan(mesh.face_offsets(), cmap)
    out = {"indices": idx, "tri_face": tri_face, "vertex_source": vsrc.astype(np.uint32)}
    if csrc is not None:
        out["corner_source"] = csrc
    if mesh.general:
        out["face_region"] = mesh.regions_of(0)
    for l in range(mesh.nlists):
        if mesh.list_target(l) > 2 or not mesh.list_fmt(l):
            continue
        rec = rows_to_records(mesh, l, vsrc, csrc)
        cols = []
        for c in range(len(cleared.list_fmt(l))):
            v = cleared.component(l, c)
            col = np.zeros(len(rec), np.float32)
            ok = rec >= 0
            col[ok] = v[rec[ok]].astype(np.float32)   # float32 -> float32 is a bit copy; doubles and integers round once
            cols.append(col)
        out[f"list{l}"] = np.stack(cols, axis=1)
    return out


def same(got, want, keys=None):
    keys = keys or sorted(want)
    assert sorted(got) == sorted(want)
    for k in keys:
        g, w = got[k], want[k]
        assert g.shape == w.shape and g.dtype == w.dtype, (k, g.shape, w.shape, g.dtype, w.dtype)
        if g.dtype == np.float32:
            g, w = g.view(np.uint32), w.view(np.uint32)
        assert np.array_equal(g, w), k


def cleared_of(cx, mesh):
    c = mesh.clone()
    if any(q for l in range(c.nlists) if c.list_target(l) <= 2 for _, q, _ in c.list_fmt(l)):
        cx.requant(c, [], clear=True)
    return c


def check_render(cx, mesh, cleared=None):
    got = cx.render_numpy(mesh)
    same(got, expected(mesh, cleared if cleared is not None else cleared_of(cx, mesh)))
    assert cx.render_stat()["ntris"] == mesh.ntri
    return got


# ---- 1. dequantisation pinned to the reference's own `-c` files
def _clear_entries():
    out = []
    for base in (GOLD, OBJ):
        man = json.load(open(os.path.join(base, "manifest.json")))
        for name, e in man.get("requant_of_hry", {}).items():
            if e["flags"] == ["-c"]:
                out.append((base, name, e["src"]))
    return out


@pytest.mark.parametrize("base,name,src", _clear_entries(), ids=[e[1] for e in _clear_entries()])
def test_dequantisation_pinned_to_reference(cx, base, name, src):
    dec = cx.read_hry(_read(os.path.join(base, src)))
    ref = cx.read_hry(_read(os.path.join(base, name + ".hry")))   # the reference's dequantised file
    got = cx.render_numpy(dec)
    want = expected(ref, ref)
    # A signed integer component does not survive the reference's lossless code (its residual code is not
    # invertible), so the decode of the `-c` file no longer holds what the dequantisation computed.  Those columns come from the
    # oracle's dequantisation of the same records, which writes the reference's `-c` file byte for byte (test_oracle_golden.py).
    signed = {(l, c) for l in range(dec.nlists) for c, (t, _, _) in enumerate(dec.list_fmt(l)) if t in (3, 5, 7, 9)}
    if signed:
        assert not dec.general
        o = op.Mesh.from_hry(_read(os.path.join(base, src)))
        o.requant([], True)
        for l, c in signed:
            want[f"list{l}"][:, c] = o.component(l, c).astype(np.float32)
    for k in want:
        if k.startswith("list"):
            assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), (name, k)
    same(got, expected(dec, cleared_of(cx, dec)))


# ---- 2. lossless goldens: the decoded records themselves
LL = sorted([os.path.join(GOLD, f) for f in os.listdir(GOLD) if f.endswith(".ll.hry")] + [os.path.join(OBJ, f) for f in os.listdir(OBJ) if f.endswith(".ll.hry")])


@pytest.mark.parametrize("path", LL, ids=[os.path.relpath(p, GOLD) for p in LL])
def test_lossless_goldens(cx, path):
    dec = cx.read_hry(_read(path))
    check_render(cx, dec, dec)
    if dec.general:   # two renders of the same mesh: identical
        a, b = cx.render_numpy(dec), cx.render_numpy(dec)
        same(a, b)


# ---- 3. triangulation
def _mixed():
    return mg.with_nonmanifold(mg.concat([mg.torus(20, 22, polys="mixed", normals=True),
                                          mg.torus(9, 11, polys="mixed", normals=True, center=(4, 0, 0)),
                                          mg.torus(8, 10, polys="mixed", normals=True, center=(-4, 0, 0))]), 4, 2)


@pytest.mark.parametrize("name", ["torus_mixed", "nonmanifold", "multi5", "tiny_tri", "meshgen_mixed"])
def test_triangulation(cx, name):
    ply = _mixed().to_ply() if name == "meshgen_mixed" else _read(os.path.join(GOLD, name + ".ply"))
    mesh = hc.Mesh.from_ply(ply)
    got = check_render(cx, mesh, mesh)
    assert got["indices"].shape == (mesh.ntri, 3) and len(got["tri_face"]) == mesh.ntri
    idx, tf = rr.fan(mesh.face_offsets(), mesh.org())
    assert np.array_equal(got["indices"], idx) and np.array_equal(got["tri_face"], tf)


# ---- 4. the same result in every profile, and from the upload path
QUANT = [(1, 0, 14), (1, 1, 14), (1, 2, 14), (1, 3, 10), (1, 4, 10), (1, 5, 10)]


def test_profiles_agree(cx):
    ply = _mixed().to_ply()
    compat = cx.write_hry(_quantised(cx, ply))
    chunked = cx.write_hry(_quantised(cx, ply), profile=hc.PROFILE_CHUNKED)
    mc = hc.MultiCodec([0])
    try:
        sharded = mc.write_hry(hc.Mesh.from_ply(ply), quants=QUANT, n_shards=3)
    finally:
        mc.close()
    assert hc.container_info(sharded)["segments"] == 3
    dec = cx.read_hry(compat)
    cleared = cleared_of(cx, dec)
    want = cx.render_numpy(dec)
    same(want, expected(dec, cleared))
    for data in (chunked, sharded):
        same(cx.render_numpy(cx.read_hry(data)), want)
        assert cx.render_stat()["uploaded_bytes"] == 0   # v0.3 decoded whole on one context: resident too
    # the upload path: the decoded mesh after hry_requant(clear), through a PLY file
    host = hc.Mesh.from_ply(cleared.to_ply())
    same(cx.render_numpy(host), want)
    assert cx.render_stat()["uploaded_bytes"] > 0


def _quantised(cx, ply):
    m = hc.Mesh.from_ply(ply)
    cx.requant(m, QUANT)
    return m


def test_quantised_double(cx):
    dec = cx.read_hry(_read(os.path.join(GOLD, "grid_double.q14.hry")))
    cleared = dec.clone()
    cx.requant(cleared, [], clear=True)
    got = cx.render_numpy(dec)
    assert [t for t, _, _ in dec.list_fmt(1)][0] == 1   # double
    same(got, expected(dec, cleared))


# ---- 5. residency
@pytest.mark.parametrize("profile", [hc.PROFILE_COMPAT, hc.PROFILE_CHUNKED])
def test_residency_ply_layout(cx, profile):
    ply = _mixed().to_ply()
    data = cx.write_hry(_quantised(cx, ply), profile=profile)
    dec = cx.read_hry(data)
    got = cx.render_numpy(dec)
    assert cx.render_stat()["uploaded_bytes"] == 0
    same(got, expected(dec, cleared_of(cx, dec)))
    # a second context uploads, with the same result
    other = hc.Codec(0)
    try:
        same(other.render_numpy(dec), got)
        assert other.render_stat()["uploaded_bytes"] > 0
    finally:
        other.close()
    # an encode of another mesh on the first context: the decode's buffers are gone, the build uploads
    dec2 = cx.read_hry(data)
    cx.write_hry(hc.Mesh.from_ply(_read(os.path.join(GOLD, "tiny_tri.ply"))))
    same(cx.render_numpy(dec2), got)
    assert cx.render_stat()["uploaded_bytes"] > 0


def test_residency_tokens_name_one_context(cx):
    # two contexts that each decode one mesh, with equal face and half-edge counts but different records: each renders the other's
    # mesh by uploading it, and gets what that mesh's own context gives
    a_mesh, b_mesh = (hc.Mesh.from_ply(mg.torus(30, 32, seed=s, normals=True).to_ply()) for s in (5, 6))
    for m in (a_mesh, b_mesh):
        cx.requant(m, QUANT)
    datas = [cx.write_hry(a_mesh, profile=hc.PROFILE_CHUNKED), cx.write_hry(b_mesh, profile=hc.PROFILE_CHUNKED)]
    ctx = [hc.Codec(0), hc.Codec(0)]
    try:
        dec = [c.read_hry(d) for c, d in zip(ctx, datas)]
        assert (dec[0].nf, dec[0].ne) == (dec[1].nf, dec[1].ne)
        assert not np.array_equal(dec[0].list_data(1), dec[1].list_data(1))
        own = []
        for c, d in zip(ctx, dec):
            own.append(c.render_numpy(d))
            assert c.render_stat()["uploaded_bytes"] == 0
        for i in (0, 1):
            other = ctx[1 - i]
            same(other.render_numpy(dec[i]), own[i])
            assert other.render_stat()["uploaded_bytes"] > 0
    finally:
        for c in ctx:
            c.close()


def test_residency_general(cx):
    sc = og.scene(mg.torus(30, 32, polys="mixed"), normals="smooth", tex="atlas", charts=5)
    data = cx.write_hry(hc.Mesh.from_obj(sc.obj, ""), profile=hc.PROFILE_CHUNKED)
    for d in (data, cx.write_hry(hc.Mesh.from_obj(sc.obj, ""))):
        dec = cx.read_hry(d)
        got = cx.render_numpy(dec)
        up = cx.render_stat()["uploaded_bytes"]
        conn = (dec.nf + 1) * 4 + dec.ne * 4
        recs = sum(dec.list_count(l) * dec.list_stride(l) for l in range(dec.nlists))
        assert up < conn + recs, (up, conn, recs)
        same(got, expected(dec, dec))
        other = hc.Codec(0)
        try:
            same(other.render_numpy(dec), got)
            assert other.render_stat()["uploaded_bytes"] > up
        finally:
            other.close()


def test_encoder_residency_untouched(cx):
    ply = _mixed().to_ply()
    data = cx.write_hry(_quantised(cx, ply), profile=hc.PROFILE_CHUNKED)
    fresh = hc.Codec(0)
    try:
        before = fresh.write_hry(fresh.read_hry(data))
    finally:
        fresh.close()
    dec = cx.read_hry(data)
    cx.render_numpy(dec)
    assert cx.write_hry(dec) == before


# ---- 6. unweld
def _scene_mesh(tmp_path, sc):
    for name, body in sc.files.items():
        (tmp_path / name).write_bytes(body)
    return hc.Mesh.from_obj(sc.obj, str(tmp_path))


SCENES = {
    "smooth_atlas": dict(normals="smooth", tex="atlas", charts=7),
    "flat": dict(normals="flat"),
    "corner_tex": dict(normals="smooth", tex="corner"),
    "materials3": dict(normals="smooth", tex="atlas", materials=3),
    "colors_some": dict(normals="smooth", tex="atlas", colors="some"),
}


def check_unweld(cx, mesh):
    got = check_render(cx, mesh, mesh)
    keys = rr.corner_keys(mesh)
    n_keys = len(np.unique(keys, axis=0))
    if rr.unwelded(mesh):
        assert cx.render_stat()["nverts"] == n_keys == len(got["vertex_source"])
        # gathering any corner list at a corner's output vertex gives that corner's own values
        cmap, _, _ = rr.vertex_map(mesh)
        for l in range(mesh.nlists):
            if mesh.list_target(l) == 2 and f"list{l}" in got:
                per_corner = rows_to_records(mesh, l, mesh.org(), np.arange(mesh.ne, dtype=np.uint32))
                vals = got[f"list{l}"][cmap]
                for c in range(vals.shape[1]):
                    comp = mesh.component(l, c).astype(np.float32)
                    w = np.where(per_corner >= 0, comp[np.maximum(per_corner, 0)], np.float32(0))
                    assert np.array_equal(vals[:, c].view(np.uint32), w.view(np.uint32))
        assert np.array_equal(got["face_region"], mesh.regions_of(0))
    same(cx.render_numpy(mesh), got)


OBJ_SRC = sorted(f for f in os.listdir(OBJ) if f.endswith(".obj") and ".dec." not in f)


@pytest.mark.parametrize("name", OBJ_SRC)
def test_unweld_obj_goldens(cx, name):
    check_unweld(cx, hc.Mesh.from_obj(_read(os.path.join(OBJ, name)), OBJ))
    hry = os.path.join(OBJ, name[:-4] + ".ll.hry")
    if os.path.exists(hry):
        check_unweld(cx, cx.read_hry(_read(hry)))


@pytest.mark.parametrize("name", sorted(SCENES))
def test_unweld_scenes(cx, tmp_path, name):
    sc = og.scene(mg.torus(24, 26, polys="mixed"), **SCENES[name])
    mesh = _scene_mesh(tmp_path, sc)
    assert rr.unwelded(mesh) or name == "colors_some"
    check_unweld(cx, mesh)
    check_unweld(cx, cx.read_hry(cx.write_hry(_scene_mesh(tmp_path, sc), profile=hc.PROFILE_CHUNKED)))


# corner counts at the edges of a wavefront of 64 (dedup.hip: one ballot per wavefront): 54 below one, 72 just above, 192 on a
# multiple; "flat": every corner of a face has a key of its own, "smooth_atlas": corners share keys
@pytest.mark.parametrize("kw", [dict(normals="flat"), dict(normals="smooth", tex="atlas")], ids=["flat", "smooth_atlas"])
@pytest.mark.parametrize("nu,nv,corners", [(3, 3, 54), (3, 4, 72), (4, 8, 192)])
def test_unweld_wavefront_edges(cx, tmp_path, nu, nv, corners, kw):
    mesh = _scene_mesh(tmp_path, og.scene(mg.torus(nu, nv), **kw))
    assert mesh.ne == corners and rr.unwelded(mesh)
    cmap, vsrc, csrc = rr.vertex_map(mesh)   # the reference handles the size, on the CPU, before the GPU is asked
    assert len(cmap) == corners and len(vsrc) == len(csrc) == len(np.unique(rr.corner_keys(mesh), axis=0))
    check_unweld(cx, mesh)


# ---- 7. scale
def test_scale_configs1(cx):
    ply = mg.torus(708, 708, seed=2, sigma=1e-4).to_ply()
    m = hc.Mesh.from_ply(ply)
    cx.requant(m, [(1, -1, 14)])
    dec = cx.read_hry(cx.write_hry(m, profile=hc.PROFILE_CHUNKED))
    assert dec.ntri == 1002528
    check_render(cx, dec)
    got = cx.render_numpy(dec)   # (check_render's requant(clear) of a clone went to this context: decode again for residency)
    dec = cx.read_hry(cx.write_hry(m, profile=hc.PROFILE_CHUNKED))
    again = cx.render_numpy(dec)
    assert cx.render_stat()["uploaded_bytes"] == 0
    same(again, got)


def test_scale_obj_scene(cx):
    sc = og.scene(mg.torus(200, 200, seed=2), normals="smooth", tex="atlas", charts=7)
    mesh = hc.Mesh.from_obj(sc.obj, "")
    assert mesh.ntri == 80000
    check_unweld(cx, mesh)


# ---- 8. refusals and torch
def test_share_refused(cx):
    ply = _mixed().to_ply()
    mc = hc.MultiCodec([0])
    try:
        data = mc.write_hry(hc.Mesh.from_ply(ply), quants=QUANT, n_shards=3)
    finally:
        mc.close()
    share = cx.read_hry(data, shard=(0, 3))
    assert share.partial
    with pytest.raises(nat.HryError) as e:
        cx.render_numpy(share)
    assert e.value.code == nat.E_ARG


TORCH_CHILD = r"""
import os, sys
import numpy as np
import torch
torch.cuda.init()   # a PyTorch program: torch holds the device before the codec starts
sys.path.insert(0, sys.argv[1])
from harry_amd import codec as hc
from harry_amd import meshgen as mg
from harry_amd import objgen as og
sc = og.scene(mg.torus(16, 18, polys="mixed"), normals="smooth", tex="atlas", materials=3)
for name, body in sc.files.items():
    open(os.path.join(sys.argv[2], name), "wb").write(body)
mesh = hc.Mesh.from_obj(sc.obj, sys.argv[2])
c = hc.Codec(0)
ref = c.render_numpy(mesh)
got = c.render(mesh)
c.close()   # the tensors outlive the context
assert sorted(got) == sorted(ref), (sorted(got), sorted(ref))
dtypes = {np.uint32: torch.int32, np.uint16: torch.int16, np.float32: torch.float32}
for k, a in ref.items():
    t = got[k]
    assert t.device == torch.device("cuda", 0) and t.dtype == dtypes[a.dtype.type] and tuple(t.shape) == a.shape, k
    assert np.array_equal(t.cpu().numpy().view(a.dtype), a), k
assert "corner_source" in got and "face_region" in got
print("torch ok")
"""


def test_torch_tensors(tmp_path):
    """Codec.render in a fresh process that uses torch first: tensors on cuda:0 with the documented dtypes and shapes, equal to
    render_numpy, readable after close()"""
    import subprocess
    import sys
    pytest.importorskip("torch")
    r = subprocess.run([sys.executable, "-c", TORCH_CHILD, util.ROOT, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "torch ok" in r.stdout, r.stdout + r.stderr
