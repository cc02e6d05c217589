"""The lever of tests/test_gpu_planes.py, pinned against the oracle without a GPU: a uchar face property written through the
oracle's face order IS a symbol plane of the container (tests/planes_ref.py), the directory carries the priors of exactly those
planes, the two chunk sizes of the 71 737-face mesh put the largest total of a stream at 65535 and 65536, and the oracle's own
chunked decode returns every designed mesh.  If one of these drifts, the GPU test no longer feeds the coders what it claims."""
import functools

import numpy as np
import pytest

from oracle import oracle_py as op
from tests import planes_ref as pr

NAMES = [n for n in pr.MESHES if n != "torus330"] + ["torus330"]


@functools.lru_cache(maxsize=None)
def built(name):
    mesh, seqs = pr.case_mesh(name)
    return op.Mesh.from_ply(mesh.to_ply()), seqs


def test_the_sequences_are_what_the_issue_designs():
    n = 71737
    s = pr.sequences(n, np.random.default_rng(1))
    assert len(s) == 8 and all(x.dtype == np.uint8 and len(x) == n for x in s)
    assert not s[0].any() and (s[1] == 255).all()
    assert np.flatnonzero(s[2]).tolist() == [1023, 1024, n - 1] and (s[2][[1023, 1024, n - 1]] == 255).all()
    assert (np.bincount(s[3], minlength=256) > 0).all()
    assert (np.diff(s[4].astype(int)) >= 0).all() and s[4][0] == 0 and s[4][-1] == 255
    assert pr.prior(np.bincount(s[4], minlength=256), n).tolist() == [4] * 256          # a chunk sees only symbols of prior 4
    b = s[5][:64 * (n // 64)].reshape(-1, 64)
    assert (np.sort(b, axis=1) == np.arange(64) * 4 + 3).all() and (b[:, 63] == 255).all()   # 64 distinct symbols, 255 in the last lane
    edges = np.flatnonzero(np.diff(s[6].astype(int)))
    assert set(np.diff(edges).tolist()) >= {62, 63, 64, 65, 66} and np.diff(edges).min() >= 62   # (equal neighbours join: longer runs)
    top = np.bincount(s[7], minlength=256)
    assert top.argmax() == 7 and 0.985 * n < top[7] < 0.995 * n and (top > 0).sum() > 200
    assert pr.prior(np.bincount(s[2], minlength=256), n)[255] == 1                      # three in 70 000: clamped to 1
    short = pr.sequences(1023, np.random.default_rng(1))
    assert np.flatnonzero(short[2]).tolist() == [1022] and pr.prior(np.bincount(short[0], minlength=256), 1023) is None
    e = pr.escape_plane(np.random.default_rng(1))
    assert np.bincount(e, minlength=256)[[10, 20, 30, 40]].tolist() == [508, 510, 512, 518]
    assert pr.prior(np.bincount(e, minlength=256), 2048)[[10, 20, 30]].tolist() == [254, 255, 256]


@pytest.mark.parametrize("name", NAMES)
def test_designed_sequences_are_the_oracles_face_symbols(name):
    """the trace of the reference-format encode: behind everything else, a record of 1 + stride symbols per coded face"""
    o, seqs = built(name)
    assert o.nf == len(seqs[0]) and o.list_stride(0) == len(seqs) and all(f == (8, 0, k) for k, f in enumerate(o.list_fmt(0)))
    res = o.clone().encode(trace=True)
    tr = res.trace()
    face = tr[(tr["ctx"] >= o.ctx_attr_base(0)) & (tr["ctx"] < o.ctx_attr_base(1))]
    assert len(face) == o.nf * (len(seqs) + 1)
    assert np.array_equal(face["sym"].reshape(o.nf, -1)[:, 1:], np.stack(seqs, 1))
    # ... and the decode returns them in that order
    assert np.array_equal(op.Mesh.from_hry(res.data).list_data(0), np.stack(seqs, 1))


@pytest.mark.parametrize("case,name,chunk,_compat", pr.CASES, ids=[c[0] for c in pr.CASES])
def test_directory_priors_and_the_oracles_chunked_decode(case, name, chunk, _compat):
    o, seqs = built(name)
    r = o.clone().encode_chunked(chunk)
    CH, CHC, nsym, tables = pr.directory(r.data, r.header_size)
    assert len(nsym) == len(tables) == pr.N_CONN_PLANES + 12 + len(seqs)    # connectivity, the bytes of x y z, the face properties
    assert CHC == min(CH, max(CH // 8, 512)) and (chunk == 0 or CH == chunk)
    for k, s in enumerate(seqs):
        p = len(nsym) - len(seqs) + k
        want = pr.prior(np.bincount(s, minlength=256), len(s))
        assert nsym[p] == len(s)
        assert (tables[p] is None) if want is None else np.array_equal(tables[p], want), (case, k)
    mixed = name.startswith("torus")
    assert nsym[12] == (o.nf if mixed else 0)                               # numtri's high byte: a zero per face, prior { 0: 1024 }
    if mixed:
        assert tables[12].tolist() == [1024] + [0] * 255
    if name == "grid33":
        assert tables[-1][[10, 20, 30, 40]].tolist() == [254, 255, 256, 259]
    ref = op.Mesh.from_hry(o.clone().encode().data)
    dec = op.Mesh.from_hry_chunked(r.data)
    assert np.array_equal(dec.org(), ref.org())
    assert np.array_equal(dec.list_data(1), ref.list_data(1))
    assert np.array_equal(dec.list_data(0), np.stack(seqs, 1))


def test_the_two_chunk_sizes_meet_and_pass_the_16_bit_limit():
    o, _ = built("torus230")
    assert o.nf == 71737
    tops = []
    for chunk in (pr.TOP_16, pr.TOP_16 + 8):
        r = o.clone().encode_chunked(chunk)
        tops.append(pr.largest_total(r.data, r.header_size))
    assert tops == [65535, 65536]
    o, _ = built("torus330")
    r = o.clone().encode_chunked(1 << 20)
    assert o.nf == 149405 and pr.largest_total(r.data, r.header_size) == 1024 + 131072
