"""Per-component error of a decode (include/harry_amd.h: hry_distortion_build), without a GPU: the restatement of
tests/distortion_ref.py on planted data, the restatement over the oracle's own quantise / encode / decode (a quantisation to q bits
costs at most half a step of the interpretation group's extent -- when the rows are paired by the numbering maps, and hundreds of
steps when they are not), and the public surface: the header declares the symbols under ABI version 6, the binding binds them."""
import math
import os
import re

import numpy as np
import pytest

from harry_amd import _native as nat
from harry_amd import codec as hc
from harry_amd import meshgen as mg
from oracle import oracle_py as op   # checker only
from tests import distortion_ref as dref
from tests import order_ref as oref
from tests.util import ROOT

NO = dref.NO
assert NO == nat.NO_ELEMENT == oref.NO
SYMBOLS = ("hry_distortion_build", "hry_distortion_component", "hry_distortion_position", "hry_distortion_get", "hry_distortion_copy",
           "hry_distortion_stat", "hry_distortion_free")


# ---- 1. planted answers
def planted():
    """12 rows of 4 components of a, 10 rows of b, a map with two rows left out and the others reversed"""
    rng = np.random.default_rng(3)
    x = rng.integers(-50, 50, size=(12, 4)).astype(np.float64)
    map_ = np.array([9, 8, NO, 7, 6, 5, 4, NO, 3, 2, 1, 0], np.uint32)
    y = np.zeros((10, 4))
    at = np.flatnonzero(map_ != NO)
    y[map_[at]] = x[at]
    return x, y, map_, at


def test_restatement_gives_the_planted_answers():
    x, y, map_, at = planted()
    y[map_[3], 0] += 2.0      # component 0: the same largest error in rows 3, 5 and 11 -- the lowest row wins -- and a smaller one
    y[map_[5], 0] -= 2.0
    y[map_[11], 0] += 2.0
    y[map_[4], 0] += 0.5
    y[map_[6], 1] = math.nan  # component 1: a NaN on b's side, an infinity on a's side, a NaN with the same bits on both
    x[8, 1] = math.inf
    x[9, 1] = y[map_[9], 1] = math.nan
    y[map_[0], 2] += 3.0      # positions = components 1..3: row 0 moves by (0, 3, 4), row 1 by (0, 0, 1)
    y[map_[0], 3] += 4.0
    y[map_[1], 3] -= 1.0
    r = dref.compare(x, y, map_, pos=1)
    c0, c1, c2, c3 = r["comp"]
    assert (c0["max_abs"], c0["argmax"], c0["sum_sq"], c0["compared"], c0["skipped"], c0["nonfinite"], c0["changed"]) == (2.0, 3, 12.25, 10, 2, 0, 4)
    assert (c0["a_min"], c0["a_max"]) == (x[at, 0].min(), x[at, 0].max())
    assert (c1["compared"], c1["nonfinite"], c1["changed"], c1["max_abs"], c1["sum_sq"]) == (7, 3, 2, 0.0, 0.0)   # (the equal NaNs: not changed)
    assert c1["argmax"] == 0                                   # all errors zero: the lowest compared row
    finite1 = [i for i in at if i not in (6, 8, 9)]
    assert (c1["a_min"], c1["a_max"]) == (x[finite1, 1].min(), x[finite1, 1].max())
    assert (c2["max_abs"], c2["argmax"], c2["changed"]) == (3.0, 0, 1) and (c3["max_abs"], c3["argmax"], c3["sum_sq"], c3["changed"]) == (4.0, 0, 17.0, 2)
    p = r["pos"]
    assert (p["max_dist"], p["argmax"], p["sum_sq_dist"], p["compared"]) == (5.0, 0, 26.0, 7)   # (rows 6, 8 and 9 have a non-finite pair)
    want_rows = np.zeros(12, np.float32)
    want_rows[[0, 1, 3, 4, 5, 11]] = [5.0, 1.0, 2.0, 0.5, 2.0, 2.0]
    assert np.array_equal(r["rows"], want_rows) and r["rows"].dtype == np.float32   # (skipped rows 2 and 7 hold 0)


def test_restatement_without_a_compared_pair():
    x = np.full((3, 1), math.nan)
    r = dref.compare(x, np.zeros((3, 1)), None, None)["comp"][0]
    assert (r["max_abs"], r["sum_sq"], r["a_min"], r["a_max"], r["compared"], r["nonfinite"], r["changed"], r["argmax"]) == (0.0, 0.0, math.inf, -math.inf, 0, 3, 3, NO)
    r = dref.compare(np.ones((2, 1)), np.ones((5, 1)), np.array([NO, NO], np.uint32))
    assert r["comp"][0]["skipped"] == 2 and r["comp"][0]["argmax"] == NO and not r["rows"].any()
    with pytest.raises(AssertionError):
        dref.compare(np.ones((2, 1)), np.ones((2, 1)), np.array([0, 2], np.uint32))   # an entry at b's count


def test_sum_tolerance_is_the_derived_bound():
    assert dref.sum_tolerance(1 << 17) == 2.0 ** -35


# ---- 2. the oracle's quantise, encode, decode: half a step of the group's extent, through the maps
@pytest.mark.parametrize("bits", [8, 12])
def test_oracle_roundtrip_costs_half_a_step(bits):
    gen = mg.torus(24, 16, normals=True)
    assert gen.verts.dtype.names == ("x", "y", "z", "nx", "ny", "nz")
    groups = ((0, 1, 2), (3, 4, 5))   # POS and NORMAL: the scale is shared over an interpretation group (quant.h:46-96)
    ply = gen.to_ply()
    src = op.Mesh.from_ply(ply)
    x = dref.values(src, 1)
    q = src.clone()
    q.requant([(1, -1, bits)])
    dec = op.Mesh.from_hry(q.encode().data)
    dec.requant([], clear=True)
    y = dref.values(dec, 1)
    m = hc.Mesh.from_ply(ply)
    w = m.clone().host_walk(plain=True)
    vertex = oref.maps_from_walk(m, w["order_v"], w["order_f"])["vertex"]
    assert not (vertex == NO).any() and not np.array_equal(vertex, np.arange(m.nv))

    def ratios(map_):
        r = dref.compare(x, y, map_, pos=0)
        out = []
        for g in groups:
            extent = max(float(x[:, c].max() - x[:, c].min()) for c in g)
            out += [r["comp"][c]["max_abs"] / (extent / (2 ** bits - 1)) for c in g]
        return r, out

    r, got = ratios(vertex)
    print(f"q{bits}: max_abs / step per component: {[round(v, 4) for v in got]}")
    assert max(got) <= 0.505, got
    assert min(got) > 0.25, got        # (a quantisation that cost nothing would be another mistake)
    assert r["pos"]["compared"] == m.nv and r["pos"]["max_dist"] <= math.sqrt(3.0) * max(c["max_abs"] for c in r["comp"][:3]) * (1 + 1e-12)
    _, wrong = ratios(None)            # the identity in place of the map: rows of different vertices
    print(f"q{bits}: with the identity: {[round(v, 1) for v in wrong]}")
    assert max(wrong) > 100.0, wrong


# ---- 3. the public surface
def test_header_declares_the_distortion_symbols_under_abi_6():
    text = open(os.path.join(ROOT, "include", "harry_amd.h")).read()
    assert re.search(r"#define\s+HRY_ABI_VERSION\s+6\b", text)
    assert re.search(r"#define\s+HRY_DISTORTION_ROWS\s+1u\b", text)
    assert "typedef struct hry_distortion hry_distortion;" in text
    assert re.search(r"\}\s*hry_comp_error;", text) and re.search(r"\}\s*hry_pos_error;", text)
    for sym in SYMBOLS:
        assert re.search(r"\b(int|void)\s+" + sym + r"\(", text), sym


def test_binding_binds_every_distortion_symbol():
    L = nat.load()
    assert L.hry_abi_version() == 6
    for sym in SYMBOLS:
        f = getattr(L, sym)
        assert f.argtypes, sym          # (bound with its argument types, not ctypes' int defaults)
        if sym != "hry_distortion_free":
            assert f.restype is nat.C.c_int, sym
    assert len(L.hry_distortion_build.argtypes) == 6 and len(L.hry_distortion_copy.argtypes) == 5
    assert nat.C.sizeof(nat.CompError) == 72 and nat.C.sizeof(nat.PosError) == 32 and nat.DISTORTION_ROWS == 1
    assert hc.Distortion.component and hc.Distortion.position and hc.Distortion.tensor and hc.Distortion.numpy and hc.Distortion.stat and hc.Distortion.close
    import inspect
    sig = inspect.signature(hc.Codec.distortion).parameters
    assert list(sig) == ["self", "src", "other", "order", "rows"] and sig["order"].default is None and sig["rows"].default is False
