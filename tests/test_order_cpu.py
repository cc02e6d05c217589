"""Numbering maps of an encode, without a GPU: the restatement of tests/order_ref.py pinned to the oracle (the source permuted by
the maps of the host walk IS the oracle's decode of its own encode, array for array -- which fixes the rotation rule of the corner
map), and the public surface: the header declares the symbols under ABI version 6, the ctypes binding binds every one of them."""
import os
import re

import numpy as np
import pytest

from harry_amd import _native as nat
from harry_amd import codec as hc
from harry_amd import meshgen as mg
from harry_amd import objgen as og
from oracle import oracle_py as op   # checker only
from tests import order_ref as oref
from tests.util import ROOT


def with_unreferenced(m: mg.Mesh, n: int = 3) -> mg.Mesh:
    """n vertices that no face names, appended"""
    extra = np.zeros(n, m.verts.dtype)
    for i, k in enumerate("xyz"):
        extra[k] = np.float32(7.0 + i) + np.arange(n, dtype=np.float32)
    return mg.Mesh(np.concatenate([m.verts, extra]), m.degrees, m.indices, m.face_props)


MESHES = {
    "torus": lambda: mg.torus(24, 16),
    "torus_mixed": lambda: mg.torus(24, 16, polys="mixed"),
    "grid_quads": lambda: mg.grid(9, 8, quads=True),
    "nonmanifold": lambda: mg.with_nonmanifold(mg.torus(12, 10)),
    "soup": lambda: mg.soup(),
    "multi": lambda: mg.multi_component(5, 8, 9),
    "multi_unreferenced": lambda: with_unreferenced(mg.multi_component(5, 8, 9)),
    "mixed_face_props": lambda: mg.with_face_props(mg.torus(12, 14, polys="mixed", normals=True)),   # (face records that differ)
}
assert oref.NO == nat.NO_ELEMENT   # (the restatement's "never coded" is the binding's HRY_NO_ELEMENT)
SYMBOLS = ("hry_order_take", "hry_order_get", "hry_order_copy", "hry_order_apply", "hry_order_free")


@pytest.mark.parametrize("name", sorted(MESHES))
def test_permuted_source_is_the_oracles_decode(name):
    ply = MESHES[name]().to_ply()
    m = hc.Mesh.from_ply(ply)
    walked = m.clone()
    w = walked.host_walk(plain=True)   # (repairs the clone's twins as an encode would)
    maps = oref.maps_from_walk(m, w["order_v"], w["order_f"])
    dec = op.Mesh.from_hry(op.Mesh.from_ply(ply).encode().data)
    want = dict(oref.decoded_arrays(dec), twin=dec.twin())
    got = oref.permuted(m, maps, twin=walked.twin())
    for key in ("face_offsets", "org", "twin", "vrec", "frec"):
        assert np.array_equal(got[key], want[key]), key
    # the maps are bijections on what is coded, and only unreferenced vertices are not
    unref = m.nv - len(np.unique(m.org()))
    assert int((maps["vertex"] == oref.NO).sum()) == unref == int((maps["vertex_inv"] == oref.NO).sum())
    for kind in ("face", "corner"):
        assert not (maps[kind] == oref.NO).any()
    for kind, rows in (("vertex", m.nv), ("face", m.nf), ("corner", m.ne)):
        x, inv = maps[kind], maps[kind + "_inv"]
        coded = np.flatnonzero(x != oref.NO)
        assert np.array_equal(inv[x[coded]], coded) and len(np.unique(x[coded])) == len(coded)
        assert np.array_equal(np.sort(x[coded]), np.arange(len(coded)))   # coded elements come first in the decoded numbering


def test_walks_with_and_without_the_operation_model_give_the_same_maps():
    """(the compat profile walks with hry_walk_run's loop, the chunked one with hry_walk_run_plain's)"""
    m = hc.Mesh.from_ply(MESHES["multi_unreferenced"]().to_ply())
    a, b = m.clone().host_walk(plain=False), m.clone().host_walk(plain=True)
    ma, mb = oref.maps_from_walk(m, a["order_v"], a["order_f"]), oref.maps_from_walk(m, b["order_v"], b["order_f"])
    assert sorted(ma) == sorted(mb) and all(np.array_equal(ma[k], mb[k]) for k in ma)


def test_header_declares_the_order_symbols_under_abi_6():
    text = open(os.path.join(ROOT, "include", "harry_amd.h")).read()
    assert re.search(r"#define\s+HRY_ABI_VERSION\s+6\b", text)
    assert re.search(r"#define\s+HRY_FLAG_ORDER\s+16\b", text) and re.search(r"#define\s+HRY_NO_ELEMENT\s+0xFFFFFFFFu", text)
    assert re.search(r"#define\s+HRY_ORDER_TO_DECODED\s+0\b", text) and re.search(r"#define\s+HRY_ORDER_TO_SOURCE\s+1\b", text)
    assert "typedef struct hry_order hry_order;" in text
    for sym in SYMBOLS:
        assert re.search(r"\b(int|void)\s+" + sym + r"\(", text), sym


def test_binding_binds_every_order_symbol():
    L = nat.load()
    assert L.hry_abi_version() == 6
    for sym in SYMBOLS:
        f = getattr(L, sym)
        assert f.argtypes, sym          # (bound with its argument types, not ctypes' int defaults)
        if sym != "hry_order_free":
            assert f.restype is nat.C.c_int, sym
    assert len(L.hry_order_apply.argtypes) == 10 and len(L.hry_order_get.argtypes) == 4
    assert (nat.FLAG_ORDER, nat.NO_ELEMENT, nat.ORDER_TO_DECODED, nat.ORDER_TO_SOURCE) == (16, 0xFFFFFFFF, 0, 1)
    assert hc.Order.to_decoded and hc.Order.to_source and hc.Order.numpy and hc.Order.tensor and hc.Order.close
    import inspect
    assert inspect.signature(hc.Codec.write_hry).parameters["return_order"].default is False


SCENES = {
    "uv_normals_materials": lambda: og.scene(mg.torus(14, 12, polys="mixed"), normals="smooth", tex="atlas", charts=4, materials=3, colors="some"),
    "normals_only": lambda: og.scene(mg.with_nonmanifold(mg.multi_component(3, 8, 9)), normals="flat"),
}


def load_scene(sc, tmp_path, cls=hc.Mesh):
    for name, body in sc.files.items():
        (tmp_path / name).write_bytes(body)
    return cls.from_obj(sc.obj, str(tmp_path))


@pytest.mark.parametrize("name", sorted(SCENES))
def test_general_bindings_permuted_source_is_the_oracles_decode(name, tmp_path):
    """records in creation order: the restatement of the record maps against the oracle's decode of its own encode"""
    sc = SCENES[name]()
    m = load_scene(sc, tmp_path)
    walked = m.clone()
    w = walked.host_walk(plain=True)
    maps = oref.maps_from_walk(m, w["order_v"], w["order_f"])
    maps.update(oref.record_maps_from_walk(m, w["order_v"], w["order_f"]))
    dec = op.Mesh.from_hry(load_scene(sc, tmp_path, op.Mesh).encode().data)
    if name == "uv_normals_materials":
        assert m.nregions(0) == 3 and m.nregions(1) == 2
    want = oref.permuted_connectivity(m, maps, walked.twin())
    for key in ("face_offsets", "org", "twin"):
        assert np.array_equal(want[key], getattr(dec, key)()), key
    oref.check_general_decode(m, dec, maps)
    for l in range(m.nlists):
        x, inv = maps[f"list{l}"], maps[f"list{l}_inv"]
        coded = np.flatnonzero(x != oref.NO)
        assert np.array_equal(inv[x[coded]], coded) and np.array_equal(np.sort(x[coded]), np.arange(len(coded)))
