"""The quantisation sweep without a GPU (include/harry_amd.h: hry_quant_sweep_build, hry_quant_choose, hry_quant_pick): the header
declares the interface under ABI version 6, the library exports it, and hry_quant_pick -- host only -- equals the restatement of
tests/quant_sweep_ref.py on designed tables.  The table itself is restated over the oracle's own requant: half a step at most where
the arithmetic is exact enough to say so."""
import ctypes as C
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
from tests import quant_sweep_ref as qref
from tests.util import ROOT

SYMBOLS = ("hry_quant_sweep_build", "hry_quant_sweep_bits", "hry_quant_sweep_component", "hry_quant_sweep_position", "hry_quant_sweep_stat",
           "hry_quant_sweep_free", "hry_quant_choose", "hry_quant_pick")
METRICS = (qref.MAX_ABS, qref.MAX_REL, qref.RMS)


def test_header_declares_the_sweep_under_abi_6():
    text = open(os.path.join(ROOT, "include", "harry_amd.h")).read()
    assert re.search(r"#define\s+HRY_ABI_VERSION\s+6\b", text)
    assert "typedef struct hry_sweep hry_sweep;" in text and re.search(r"\}\s*hry_tolerance;", text)
    assert re.search(r"enum\s*\{\s*HRY_TOL_MAX_ABS\s*=\s*0,\s*HRY_TOL_MAX_REL\s*=\s*1,\s*HRY_TOL_RMS\s*=\s*2,\s*HRY_TOL_POS_DIST\s*=\s*3\s*\}", text)
    for sym in SYMBOLS:
        assert re.search(r"\b(int|void)\s+" + sym + r"\(", text), sym
    assert "hry_quant_sweep_build (no counterpart" in text   # the list of entry points at the top


def test_library_exports_and_binding_binds_the_sweep():
    L = nat.load()
    assert L.hry_abi_version() == 6
    raw = C.CDLL(nat.LIB_PATH)
    for sym in SYMBOLS:
        assert getattr(raw, sym), sym
        f = getattr(L, sym)
        assert f.argtypes, sym
        if sym != "hry_quant_sweep_free":
            assert f.restype is C.c_int, sym
    assert C.sizeof(nat.Tolerance) == 24 and (nat.TOL_MAX_ABS, nat.TOL_MAX_REL, nat.TOL_RMS, nat.TOL_POS_DIST) == (0, 1, 2, 3)
    for name in ("bits", "component", "position", "table", "choose", "stat", "close"):
        assert callable(getattr(hc.QuantSweep, name)), name
    assert callable(hc.Codec.quant_sweep)


# ---- hry_quant_pick against the restatement, on designed tables
def rec(max_abs, sum_sq=None, compared=100):
    return {"max_abs": float(max_abs), "sum_sq": float(max_abs * max_abs * compared / 3 if sum_sq is None else sum_sq), "compared": compared}


def native_pick(table, metric, extent, value, n_bits=None):
    n = len(table) if n_bits is None else n_bits
    arr = (nat.CompError * max(n, 1))()
    for i, r in enumerate(table[:max(n, 0)]):
        arr[i].max_abs, arr[i].sum_sq, arr[i].compared = r["max_abs"], r["sum_sq"], r["compared"]
        arr[i].a_min, arr[i].a_max, arr[i].argmax = 0.0, 1.0, 0
    return nat.load().hry_quant_pick(arr, n, metric, extent, value)


def monotone(n):
    return [rec(8.0 / (2 ** q - 1) / 2) for q in range(1, n + 1)]


def dipped(n=12):
    """the error at 9 bits above the error at 8 bits: the table is not monotone"""
    t = monotone(n)
    t[8] = rec(t[7]["max_abs"] * 1.5)
    assert t[8]["max_abs"] > t[7]["max_abs"] > t[9]["max_abs"]
    return t


def agree(table, metric, extent, value):
    want = qref.pick(table, metric, extent, value)
    got = native_pick(table, metric, extent, value)
    assert got == want, (metric, extent, value, got, want)
    return got


@pytest.mark.parametrize("n_bits", [1, 8, 16, 30])
def test_pick_on_a_monotone_table(n_bits):
    t = monotone(n_bits)
    extent = 8.0
    for q in range(1, n_bits + 1):
        e = t[q - 1]["max_abs"]
        assert agree(t, qref.MAX_ABS, extent, e) == q                       # a tolerance of exactly max_abs is met
        assert agree(t, qref.MAX_ABS, extent, math.nextafter(e, 0.0)) == (q + 1 if q < n_bits else 0)
        assert agree(t, qref.MAX_REL, extent, e / extent) == qref.pick(t, qref.MAX_ABS, extent, (e / extent) * extent)
        rms = math.sqrt(t[q - 1]["sum_sq"] / t[q - 1]["compared"])
        assert agree(t, qref.RMS, extent, rms) == q
    for metric in METRICS:
        assert agree(t, metric, extent, 0.0) == 0                           # no width meets it
        assert agree(t, metric, extent, 1e9) == 1
    assert native_pick(t, qref.MAX_ABS, extent, 1e9, n_bits=0) == 0          # an empty table: none does


def test_pick_takes_the_first_width_that_meets_it_on_a_table_with_a_dip():
    t = dipped()
    between = (t[7]["max_abs"] + t[8]["max_abs"]) / 2    # met at 8 bits, violated at 9, met again from 10
    assert agree(t, qref.MAX_ABS, 8.0, between) == 8
    assert not qref.meets(t[8], qref.MAX_ABS, 8.0, between) and qref.meets(t[9], qref.MAX_ABS, 8.0, between)
    below = math.nextafter(t[7]["max_abs"], 0.0)          # violated at 8 and 9: the pick jumps the dip
    assert agree(t, qref.MAX_ABS, 8.0, below) == 10
    assert agree(t, qref.MAX_REL, 8.0, between / 8.0) == qref.pick(t, qref.MAX_REL, 8.0, between / 8.0) in (8, 10)
    assert agree(t, qref.RMS, 8.0, math.sqrt(t[7]["sum_sq"] / t[7]["compared"])) == 8


def test_pick_under_rms_needs_a_compared_pair():
    t = [rec(0.0, 0.0, compared=0), rec(0.0, 0.0, compared=0), rec(0.25, 1.0, compared=16)]
    assert agree(t, qref.RMS, 1.0, 0.25) == 3             # the empty records do not meet an RMS tolerance, whatever it is
    assert agree(t, qref.RMS, 1.0, 0.2) == 0
    assert agree(t, qref.MAX_ABS, 1.0, 0.0) == 1          # ... but their max_abs of 0 meets MAX_ABS
    assert agree(t[:2], qref.RMS, 1.0, 1e300) == 0


def test_pick_refuses_what_is_no_tolerance():
    t = monotone(8)
    for metric in METRICS:
        for value in (-1.0, -1e-300, math.nan, -math.inf):
            assert native_pick(t, metric, 8.0, value) == nat.E_ARG, (metric, value)
            assert nat.load().hry_last_error()
    assert native_pick(t, qref.POS_DIST, 8.0, 1.0) == nat.E_ARG     # a component's record has no distance
    assert native_pick(t, 17, 8.0, 1.0) == nat.E_ARG
    assert native_pick(t, qref.MAX_ABS, 8.0, 1.0, n_bits=-1) == nat.E_ARG
    assert native_pick(t, qref.MAX_ABS, 8.0, math.inf) == 1         # (an infinite tolerance is one)


# ---- the table over the oracle's requant: what the sweep restates, without a device
def test_oracle_table_costs_half_a_step_and_pick_finds_the_width():
    gen = mg.torus(24, 16, normals=True)
    src = op.Mesh.from_ply(gen.to_ply())
    x = dref.values(src, 1)
    extent = max(float(x[:, c].max() - x[:, c].min()) for c in (0, 1, 2))   # shared over the POS group (quant.h:46-96)
    widths = 12

    def values_at(comps, bits):
        return qref.oracle_values(src, 1, comps, bits)

    t = qref.table(values_at, x, 0, widths)
    assert len(t) == widths and all(r["compared"] == len(x) and r["skipped"] == 0 for r in t)
    for q, r in enumerate(t, 1):
        step = extent / (2 ** q - 1)
        print(f"q{q}: max_abs / step = {r['max_abs'] / step:.4f}")
        assert r["max_abs"] <= 0.505 * step    # (float arithmetic: a little over half a step at the wide end)
    tol = (t[9]["max_abs"] + t[10]["max_abs"]) / 2
    assert t[10]["max_abs"] < tol < t[9]["max_abs"] and qref.pick(t, qref.MAX_ABS, extent, tol) == 11
    assert native_pick(t, qref.MAX_ABS, extent, tol) == 11 and native_pick(t, qref.MAX_REL, extent, tol / extent) == qref.pick(t, qref.MAX_REL, extent, tol / extent)
    p = qref.position_table(values_at, x, 0, 4)
    for q, r in enumerate(p, 1):
        assert r["compared"] == len(x) and r["max_dist"] <= math.sqrt(3.0) * 0.505 * extent / (2 ** q - 1)
