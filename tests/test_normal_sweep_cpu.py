"""The faces' normal deviation without a GPU (include/harry_amd.h: hry_normal_error, hry_quant_sweep_build_ex, hry_distortion_normals,
hry_chord_angle / hry_angle_chord): the header declares the interface under ABI version 6, the library exports it, the two host
helpers are each other's inverse and refuse what is no chord or angle -- and the meshes of tests/test_gpu_normal_sweep.py demand what
they are there for, against the oracle's requant alone (tests/normal_error_ref.py).  hry_quant_choose has no entry without a device
(its handle comes out of a build): the metric is tested in tests/test_gpu_normal_sweep.py."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from harry_amd import _native as nat
from harry_amd import codec as hc
from oracle import oracle_py as op   # checker only
from tests import distortion_ref as dref
from tests import normal_error_ref as nref
from tests import quant_sweep_ref as qref
from tests.util import ROOT

SYMBOLS = ("hry_quant_sweep_build_ex", "hry_quant_sweep_normals", "hry_distortion_normals", "hry_chord_angle", "hry_angle_chord")
ANGLES_DEG = (10.0, 1.0, 0.025)


def test_header_declares_the_normals_under_abi_6():
    text = open(os.path.join(ROOT, "include", "harry_amd.h")).read()
    assert re.search(r"#define\s+HRY_ABI_VERSION\s+6\b", text)
    assert re.search(r"\}\s*hry_normal_error;", text)
    assert re.search(r"#define\s+HRY_DISTORTION_NORMALS\s+4u", text) and re.search(r"#define\s+HRY_SWEEP_NORMALS\s+1u", text)
    assert re.search(r"HRY_TOL_NORMAL_CHORD\s*=\s*4\b", text)
    for sym in SYMBOLS:
        assert re.search(r"\bint\s+" + sym + r"\(", text), sym


def test_library_exports_and_binding_binds_the_normals():
    L = nat.load()
    assert L.hry_abi_version() == 6
    raw = C.CDLL(nat.LIB_PATH)
    for sym in SYMBOLS:
        assert getattr(raw, sym), sym
        f = getattr(L, sym)
        assert f.argtypes and f.restype is C.c_int, sym
    assert C.sizeof(nat.NormalError) == 64
    assert (nat.DISTORTION_ROWS, nat.DISTORTION_NORMALS, nat.SWEEP_NORMALS, nat.TOL_NORMAL_CHORD) == (1, 4, 1, 4)
    assert callable(hc.QuantSweep.normals) and callable(hc.Distortion.normals) and callable(hc.Codec.distortion_ex) and hc.QuantSweep.METRICS["normal_chord"] == 4


def test_chord_and_angle_are_each_others_inverse():
    for deg in (0.0, 1e-6, 0.025, 1.0, 10.0, 60.0, 90.0, 179.0, 180.0):
        rad = math.radians(deg)
        chord = hc.angle_chord(rad)
        assert chord == 2.0 * math.sin(rad / 2.0)
        back = hc.chord_angle(chord)
        assert back == 2.0 * math.asin(min(chord / 2.0, 1.0))
        # asin is ill-conditioned at 1: the angle comes back to a relative 2^-50 up to 90 degrees, to sqrt(2^-52) at 180
        assert abs(back - rad) <= (2.0 ** -50 * rad if deg <= 90.0 else 2.0 ** -25)
    assert hc.chord_angle(0.0) == 0.0 and hc.chord_angle(2.0) == math.pi
    assert hc.chord_angle(2.0000001) == math.pi and hc.chord_angle(math.inf) == math.pi   # (min(chord / 2, 1))
    assert hc.angle_chord(math.pi) == 2.0


def test_chord_and_angle_refuse_what_is_neither():
    L = nat.load()
    out = C.c_double(-7.0)
    for bad in (-1.0, -1e-300, math.nan, -math.inf):
        assert L.hry_chord_angle(bad, C.byref(out)) == nat.E_ARG and L.hry_last_error()
        assert L.hry_angle_chord(bad, C.byref(out)) == nat.E_ARG and L.hry_last_error()
    for bad in (math.nextafter(math.pi, 4.0), 4.0, math.inf):
        assert L.hry_angle_chord(bad, C.byref(out)) == nat.E_ARG
    assert L.hry_chord_angle(1.0, None) == nat.E_ARG and L.hry_angle_chord(1.0, None) == nat.E_ARG
    assert out.value == -7.0   # (nothing written on a refusal)
    with pytest.raises(hc.HryError):
        hc.angle_chord(4.0)


# ---- the cases demand what they are there for: against the oracle alone
def oracle_table(name: str, qmax: int) -> list:
    g = nref.mesh(name)
    src = op.Mesh.from_ply(g.to_ply())
    x = dref.values(src, 1)
    return nref.table(lambda comps, bits: qref.oracle_values(src, 1, comps, bits), x, 0, qmax, g.degrees, g.indices)


def tri_widths(tab: list) -> list:
    """the widths the three angles pick on tri's table"""
    return [nref.pick(tab, nref.chord_of_degrees(d)) for d in ANGLES_DEG]


def test_tri_collapses_at_low_widths_and_three_angles_pick_three_widths():
    g = nref.mesh("tri")
    assert (g.nv, g.nf) == (1600, 3200) and (g.degrees == 3).all()
    tab = oracle_table("tri", 30)
    for q, r in enumerate(tab, 1):
        print(q, {k: r[k] for k in nref.FIELDS})
    assert all(tab[q - 1]["collapsed"] > 0 for q in (1, 2, 3))
    first_whole = next(q for q, r in enumerate(tab, 1) if r["collapsed"] == 0)
    assert first_whole <= 12
    widths = tri_widths(tab)
    print("widths for", ANGLES_DEG, "degrees:", widths)
    assert len(set(widths)) == 3 and all(1 < w < 30 for w in widths)
    assert widths == sorted(widths)
    for w, d in zip(widths, ANGLES_DEG):   # the choice rule: met at the width, not met at any narrower one
        assert nref.meets(tab[w - 1], nref.chord_of_degrees(d)) and not any(nref.meets(r, nref.chord_of_degrees(d)) for r in tab[:w - 1])


def test_bad_has_nonfinite_and_degenerate_faces():
    tab = oracle_table("bad", 12)
    for r in tab:
        assert r["nonfinite"] >= 4 and r["degenerate"] >= 2 and r["skipped"] == 0
    # with an infinite x as well the POS group's shared extent is infinite: every position requantises to a NaN, at every width
    g = nref.mesh("bad_inf")
    for r in oracle_table("bad_inf", 3):
        assert r["nonfinite"] == g.nf
    # ... while a comparison that does not requantise sees the two vertices' faces only
    x = dref.values(op.Mesh.from_ply(g.to_ply()), 1)[:, :3]
    same = nref.compare(x, x, g.degrees, g.indices)
    assert same["nonfinite"] == 12 and same["degenerate"] >= 2 and same["max_chord"] == 0.0 and same["compared"] > 3000


def test_mixed_holds_every_degree_and_the_types_their_widths():
    g = nref.mesh("mixed")
    assert set(np.unique(g.degrees).tolist()) == {3, 4, 5, 64}
    assert int(g.degrees[-1]) == 64 and g.nv == 24 * 24 + 64
    tab = oracle_table("mixed", 8)
    assert tab[0]["collapsed"] > 0 and tab[7]["collapsed"] == 0 and tab[7]["compared"] == g.nf
    for name, dt in (("ushort", np.uint16), ("int", np.int32), ("double", np.float64)):
        v = nref.mesh(name).verts
        assert all(v.dtype[k] == dt for k in "xyz"), name


def test_reference_classes_in_order_and_through_maps():
    """the restatement itself on a face of every class: one triangle each, through a map and a row table"""
    x = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 2, 2], [np.nan, 0, 0], [5, 5, 5]], np.float64)
    y = x.copy()
    y[2] = [0, 1, 1]            # tilts face 0 by 45 degrees
    deg = np.array([3, 3, 3, 3, 3], np.uint8)
    idx = np.array([0, 1, 2,  0, 1, 4,  3, 3, 3,  0, 1, 5,  0, 2, 1], np.uint32)
    map_ = np.arange(6, dtype=np.uint32)
    map_[5] = nref.NO
    r = nref.compare(x, y, deg, idx, map_)
    assert (r["compared"], r["nonfinite"], r["degenerate"], r["skipped"], r["collapsed"]) == (2, 1, 1, 1, 0)
    assert r["argmax"] == 0 and abs(r["max_chord"] - nref.chord_of_degrees(45.0)) < 1e-15
    assert r["faces"][0] == np.float32(r["max_chord"]) and r["faces"][4] == r["faces"][0] and not r["faces"][1:4].any()
    y[:3] = [[0, 0, 0], [1, 0, 0], [2, 0, 0]]   # the quantisation put face 0 on a line
    assert nref.compare(x, y, deg, idx, map_)["collapsed"] == 2
    rows = np.array([0, 1, 2, 3, 4, nref.NO], np.uint32)   # vertex 5 has no row: skipped before anything is read
    assert nref.compare(x, y, deg, idx, rows=rows)["skipped"] == 1
