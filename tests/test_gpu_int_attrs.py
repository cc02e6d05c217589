"""Integer attributes of every PLY type (char, uchar, short, ushort, int, uint) at the limits of their ranges, on the device:
prediction, residuals and reconstruction (k_predict_vtx, k_face_planes, k_residuals_to_rec, k_faces_unfold, k_unpredict2,
k_unpredict3), bounds, quantiser and dequantiser (k_bounds_*, k_requant, dequantise_bits) and the render columns.

The reference's answers: tests/golden/int_*.{ply,hry,dec.ply} flow through the parametrisations of test_gpu_parity, test_gpu_chunked,
test_gpu_configs and test_gpu_render; here the same value classes on meshes of several blocks and slices, against the CPU oracle
(byte-pinned to the reference on those fixtures) and the reference's own hashes in the manifest's "big" section.  Every comparison
is exact."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

from harry_amd import _native as nat
from harry_amd import codec as hc
from harry_amd import meshgen as mg
from oracle import oracle_py as op
from tests import render_ref as rr
from tests import util

pytestmark = pytest.mark.gpu

GOLD = os.path.join(util.ROOT, "tests", "golden")
with open(os.path.join(GOLD, "manifest.json")) as _f:
    MANIFEST = json.load(_f)
# every quantisation the reference answered on integer attributes: (fixture.tag, flags)
QUANTS = [(f"{n}.{t}", v["flags"]) for n, e in sorted(MANIFEST["small"].items()) if n.startswith("int_")
          for t, v in sorted(e["variants"].items()) if v["flags"]]


@pytest.fixture(scope="module")
def cx():
    c = hc.Codec(0)
    yield c
    c.close()


def same_mesh(a, b):
    assert (a.nv, a.nf, a.ne) == (b.nv, b.nf, b.ne)
    assert np.array_equal(a.face_offsets(), b.face_offsets())
    assert np.array_equal(a.org(), b.org())
    for l in range(2):
        assert a.list_fmt(l) == b.list_fmt(l)
        assert np.array_equal(a.list_data(l), b.list_data(l)), f"list {l} differs"


# ---- (a), (b): lossless, vertex and face lists, records whose wide components lie at odd offsets ------------------------------------
@pytest.mark.parametrize("name", sorted(util.INT_BIG_CASES))
def test_lossless_integer_attributes(cx, name, monkeypatch):
    """both profiles' bytes equal the oracle's -- the compat stream's hash the one the reference wrote -- and both decode to the
    oracle's decode of the reference-format stream: in one piece, and pipelined in slices small and large"""
    e = MANIFEST["big"][name]
    ply = util.INT_BIG_CASES[name]().to_ply()
    assert hashlib.sha256(ply).hexdigest() == e["ply_sha256"], "not the input the reference answered (tests/golden/make_golden.py)"
    a, o = hc.Mesh.from_ply(ply), op.Mesh.from_ply(ply)
    want = o.clone().encode().data
    compat = cx.write_hry(a.clone(), profile=hc.PROFILE_COMPAT)
    assert compat == want
    assert (len(compat), hashlib.sha256(compat).hexdigest()) == (e["variants"]["ll"]["hry_bytes"], e["variants"]["ll"]["hry_sha256"])
    chunked = cx.write_hry(a.clone(), profile=hc.PROFILE_CHUNKED)
    assert chunked == o.clone().encode_chunked(0).data
    ref_dec = op.Mesh.from_hry(want)
    for stream in (compat, chunked):
        same_mesh(cx.read_hry(stream), ref_dec)
    monkeypatch.setenv("HRY_NO_PIPELINE", "1")
    for stream in (compat, chunked):
        same_mesh(cx.read_hry(stream), ref_dec)
    monkeypatch.delenv("HRY_NO_PIPELINE")
    monkeypatch.setenv("HRY_PIPELINE_MIN_VERTICES", "0")
    for faces, slice_ in ((64, 64), (1000, 4096)):
        monkeypatch.setenv("HRY_PIPELINE_FACES", str(faces))
        monkeypatch.setenv("HRY_PIPELINE_SLICE", str(slice_))
        for stream in (compat, chunked):
            same_mesh(cx.read_hry(stream), ref_dec)


# ---- (c): bounds, quantiser, dequantiser, render columns ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _quant_ply(values):
    return mg.with_integer_props(mg.torus(70, 75, seed=5), values=values, face=True).to_ply()


def _first_extremes(m, l):
    """per component (1 + the first element holding the minimum, the same for the maximum), as Mesh.bounds_at counts them.  The
    values here never equal the scan's initial ones (the type's greatest value as minimum, its least as maximum), which count 0."""
    n = len(m.list_fmt(l))
    return [(1 + int(np.argmin(m.component(l, c))), 1 + int(np.argmax(m.component(l, c)))) for c in range(n)]


@pytest.mark.parametrize("values", ["half", "full"])
@pytest.mark.parametrize("case,flags", QUANTS, ids=[c for c, _ in QUANTS])
def test_quantised_integer_attributes(cx, values, case, flags):
    """every (type, width) the reference answered in tests/golden/manifest.json, on values over half and over the whole of each
    type: bounds and where they lie, the quantised records, the dequantised records, the render columns"""
    ply = _quant_ply(values)
    a, o = hc.Mesh.from_ply(ply), op.Mesh.from_ply(ply)
    quant, clear = util.flags_to_quant(flags)
    cx.bounds(a)
    for l in range(2):
        assert np.array_equal(a.list_min(l), o.list_min(l)) and np.array_equal(a.list_max(l), o.list_max(l)), l
        assert a.bounds_at(l) == _first_extremes(o, l), l
    cx.requant(a, quant, clear)
    o.requant(quant, clear)
    for l in range(2):
        assert a.list_fmt(l) == o.list_fmt(l)
        assert np.array_equal(a.list_data(l), o.list_data(l)), f"quantised list {l}"
    oc = o.clone()
    oc.requant([], True)
    got = cx.render_numpy(a)
    idx, tri_face = rr.fan(a.face_offsets(), a.org())
    assert np.array_equal(got["indices"], idx) and np.array_equal(got["tri_face"], tri_face)
    for l in range(2):
        want = np.stack([oc.component(l, c).astype(np.float32) for c in range(len(oc.list_fmt(l)))], axis=1)
        assert np.array_equal(got[f"list{l}"].view(np.uint32), want.view(np.uint32)), f"render columns of list {l}"
    ac = a.clone()
    cx.requant(ac, [], clear=True)
    for l in range(2):
        assert ac.list_fmt(l) == oc.list_fmt(l)
        assert np.array_equal(ac.list_data(l), oc.list_data(l)), f"dequantised list {l}"


# ---- quantised values through the codec: a signed source leaves values above 2^q - 1 in its unsigned storage word ----------------------
@pytest.mark.parametrize("case", ["int_full.q6", "int_half.q17", "int_half.mixed"])
def test_quantised_signed_sources_through_the_codec(cx, case, monkeypatch):
    """Values over the whole of every type, quantised, at 5 250 vertices (several batches and ring reloads; the oracle's bytes equal
    the reference's on this input at every width of the manifest).  q6: every component in 8-bit storage, the three signed ones
    with values above 63 -- the list must not go through the forms that rest on values <= 2^q - 1 (k_unpredict3, the pipelined
    slices, LaneEvalSmall); q17: the same in 32-bit storage; mixed: 8-, 16- and 32-bit storage in one record.  Both profiles'
    bytes equal the oracle's and decode to its decode of the reference-format stream: plain, and with the pipelined decode forced."""
    n, t = case.split(".")
    quant, clear = util.flags_to_quant(MANIFEST["small"][n]["variants"][t]["flags"])
    ply = _quant_ply("full")
    a, o = hc.Mesh.from_ply(ply), op.Mesh.from_ply(ply)
    cx.requant(a, quant, clear)
    o.requant(quant, clear)
    if case == "int_full.q6":   # (the case is about values above the top of their width)
        assert all(int(o.component(1, c).max()) > 63 for c in (3, 5, 7)) and all(q == 6 for _, q, _ in o.list_fmt(1))
    want = o.clone().encode().data
    compat = cx.write_hry(a.clone(), profile=hc.PROFILE_COMPAT)
    assert compat == want
    chunked = cx.write_hry(a.clone(), profile=hc.PROFILE_CHUNKED)
    assert chunked == o.clone().encode_chunked(0).data
    ref_dec = op.Mesh.from_hry(want)
    monkeypatch.setenv("HRY_NO_PIPELINE", "1")
    for stream in (compat, chunked):
        same_mesh(cx.read_hry(stream), ref_dec)
    monkeypatch.delenv("HRY_NO_PIPELINE")
    monkeypatch.setenv("HRY_PIPELINE_MIN_VERTICES", "0")
    for faces, slice_ in ((64, 64), (1000, 4096)):
        monkeypatch.setenv("HRY_PIPELINE_FACES", str(faces))
        monkeypatch.setenv("HRY_PIPELINE_SLICE", str(slice_))
        for stream in (compat, chunked):
            same_mesh(cx.read_hry(stream), ref_dec)


# ---- (d): the extent the reference cannot divide by --------------------------------------------------------------------------------
def test_int_over_the_whole_type_is_refused(cx):
    """An `int` component that holds the type's least and greatest value: max - min wraps to -1, and the value 0 lies the type's
    least value above the minimum -- the reference's quantiser divides the one by the other (quant.h:106) and dies of SIGFPE (the
    oracle restates that division: this input is never handed to it here).  The product refuses the request, like a zero extent,
    and goes on working."""
    v = np.zeros(4, dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("p", "<i4")])
    v["x"], v["y"] = [0, 1, 1, 0], [0, 0, 1, 1]
    v["p"] = [np.iinfo(np.int32).min, np.iinfo(np.int32).max, 0, 5]
    ply = mg.Mesh(v, np.full(2, 3, np.uint8), np.array([0, 1, 2, 0, 2, 3], np.uint32)).to_ply()
    m = hc.Mesh.from_ply(ply)
    with pytest.raises(hc.HryError) as err:
        cx.requant(m, [(1, 3, 8)])
    assert err.value.code == nat.E_UNSUPPORTED
    # ... lossless it is an input like any other, to the reference and the oracle too: the division is the quantiser's
    # (quant.h:106), and a lossless encode never rescales -- the one call here that may take this input in-process
    assert cx.write_hry(hc.Mesh.from_ply(ply)) == op.Mesh.from_ply(ply).encode().data
    # ... and the context still quantises and encodes a fixture
    ply = open(os.path.join(GOLD, "int_half.ply"), "rb").read()
    a = hc.Mesh.from_ply(ply)
    quant, clear = util.flags_to_quant(MANIFEST["small"]["int_half"]["variants"]["mixed"]["flags"])
    cx.requant(a, quant, clear)
    assert cx.write_hry(a) == open(os.path.join(GOLD, "int_half.mixed.hry"), "rb").read()
