"""The rate sweep without a GPU (include/harry_amd.h: hry_rate_sweep_build, hry_rate_hist_bytes, hry_rate_pick, hry_rate_choose): the
header declares the interface under ABI version 6, the library exports it and the binding binds it, and the two host-only functions
equal the restatement of tests/rate_sweep_ref.py.  The entropy's tolerance is 1e-12 relative -- derived, not measured: at most 256
positive terms, each a few ulps (2^-52) from its exact value, summed in double."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from harry_amd import _native as nat
from harry_amd import codec as hc
from tests import rate_sweep_ref as rref
from tests.util import ROOT

SYMBOLS = ("hry_rate_sweep_build", "hry_rate_sweep_coded", "hry_rate_sweep_bits", "hry_rate_sweep_planes", "hry_rate_sweep_hist", "hry_rate_sweep_bytes",
           "hry_rate_sweep_stat", "hry_rate_sweep_free", "hry_rate_hist_bytes", "hry_rate_pick", "hry_rate_choose")
REL = 1e-12


def test_header_declares_the_rate_sweep_under_abi_6():
    text = open(os.path.join(ROOT, "include", "harry_amd.h")).read()
    assert re.search(r"#define\s+HRY_ABI_VERSION\s+6\b", text)
    assert "typedef struct hry_rate_sweep hry_rate_sweep;" in text
    for sym in SYMBOLS:
        assert re.search(r"\b(int|void|uint32_t)\s+" + sym + r"\(", text), sym
    assert "hry_rate_sweep_build (no counterpart" in text   # the list of entry points at the top


def test_library_exports_and_binding_binds_the_rate_sweep():
    L = nat.load()
    assert L.hry_abi_version() == 6
    raw = C.CDLL(nat.LIB_PATH)
    for sym in SYMBOLS:
        assert getattr(raw, sym), sym
        f = getattr(L, sym)
        assert f.argtypes, sym
        if sym == "hry_rate_sweep_coded":
            assert f.restype is C.c_uint32
        elif sym != "hry_rate_sweep_free":
            assert f.restype is C.c_int, sym
    for name in ("coded", "bits", "hist", "bytes", "choose", "stat", "close"):
        assert hasattr(hc.RateSweep, name), name
    assert callable(hc.Codec.rate_sweep) and callable(hc.rate_hist_bytes) and callable(hc.rate_pick)


def close(got: float, want: float) -> bool:
    return abs(got - want) <= REL * abs(want)


def hist(**counts):
    h = np.zeros(256, np.uint32)
    for k, v in counts.items():
        h[int(k[1:])] = v
    return h


def test_hist_bytes_on_designed_histograms():
    assert hc.rate_hist_bytes(np.zeros(256, np.uint32)) == 0.0                       # empty
    for sym, n in ((0, 1), (17, 1000), (255, 2 ** 32 - 1)):                         # one symbol: no information
        h = np.zeros(256, np.uint32)
        h[sym] = n
        assert hc.rate_hist_bytes(h) == 0.0 == rref.hist_bytes(h)
    for n in (2, 1000, 2 ** 31):                                                    # two equal symbols: a bit each, exactly
        assert hc.rate_hist_bytes(hist(s3=n // 2, s200=n // 2)) == n / 8
    for k in (1, 7, 4096, 2 ** 24 - 1):                                             # uniform over 256: a byte each, exactly
        assert hc.rate_hist_bytes(np.full(256, k, np.uint32)) == 256 * k
    assert close(hc.rate_hist_bytes(hist(s0=3, s1=1)), (3 * math.log2(4 / 3) + 2) / 8)


@pytest.mark.parametrize("seed", range(6))
def test_hist_bytes_on_random_histograms(seed):
    rng = np.random.default_rng(seed)
    h = rng.integers(0, (1, 50, 100000, 2 ** 24, 3, 1000)[seed] + 1, 256).astype(np.uint32)
    if seed == 4:
        h[rng.integers(0, 256, 200)] = 0                                            # a sparse one
    if seed == 5:
        h = (rng.geometric(0.05, 256) * (rng.random(256) < 0.3)).astype(np.uint32)   # skewed
    got, want = hc.rate_hist_bytes(h), rref.hist_bytes(h)
    print(f"seed {seed}: n {int(h.sum())} got {got!r} want {want!r}")
    assert close(got, want) and 0.0 <= got <= int(h.sum()) * (1 + REL)
    with pytest.raises(hc.HryError):
        hc.rate_hist_bytes(h[:100])


def test_pick_is_the_largest_width_that_fits():
    t = [10.0 * q for q in range(1, 31)]
    for budget in (0.0, 9.99, 10.0, 10.01, 155.0, 300.0, 1e9, math.inf):
        assert hc.rate_pick(t, budget) == rref.pick(t, budget)
    assert hc.rate_pick(t, 10.0) == 1 and hc.rate_pick(t, 9.99) == 0 and hc.rate_pick(t, 300.0) == 30 and hc.rate_pick(t, 155.0) == 15
    assert hc.rate_pick(t, 1e9, n_bits=12) == 12 and hc.rate_pick(t, 1e9, n_bits=0) == 0 and hc.rate_pick([], 5.0) == 0


def test_pick_on_a_table_that_is_not_monotone():
    t = [10.0, 20.0, 50.0, 30.0, 60.0, 45.0, 90.0]          # 4 bits cheaper than 3, 6 cheaper than 5
    assert hc.rate_pick(t, 47.0) == 6 == rref.pick(t, 47.0)   # the largest that fits, though 5 bits do not
    assert hc.rate_pick(t, 35.0) == 4 == rref.pick(t, 35.0)   # ... and 3 bits do not
    assert hc.rate_pick(t, 25.0) == 2 and hc.rate_pick(t, 5.0) == 0
    for budget in np.arange(0.0, 100.0, 2.5):
        assert hc.rate_pick(t, budget) == rref.pick(t, budget)


def test_pick_refuses_what_is_no_budget():
    t = [1.0, 2.0, 3.0]
    for budget in (-1.0, -1e-300, math.nan, -math.inf):
        with pytest.raises(hc.HryError) as e:
            hc.rate_pick(t, budget)
        assert e.value.code == nat.E_ARG and nat.load().hry_last_error()
    with pytest.raises(hc.HryError) as e:
        hc.rate_pick(t, 1.0, n_bits=-1)
    assert e.value.code == nat.E_ARG
    L = nat.load()
    assert L.hry_rate_pick(None, 3, 1.0) == nat.E_ARG and L.hry_rate_pick(None, 0, 1.0) == 0
    out = C.c_double()
    assert L.hry_rate_hist_bytes(None, C.byref(out)) == nat.E_ARG
    bits = C.c_int(5)
    assert L.hry_rate_choose(None, 1, 0, 1.0, C.byref(bits), None) == nat.E_ARG and bits.value == 0
    assert L.hry_rate_sweep_coded(None) == 0 and L.hry_rate_sweep_bits(None, 1, 0) == nat.E_ARG
    L.hry_rate_sweep_free(None)
