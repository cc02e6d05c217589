"""The designed meshes of tests/seam_meshes.py on the restatements alone: every case reaches the seam it is there for -- counted on the
arrays, never measured on a kernel -- and has the headline numbers its design gives.  tests/test_gpu_seams.py asserts the same
conditions again on a render build's buffers and compares the kernels in full."""
import numpy as np
import pytest

from tests import edges_ref as er
from tests import orient_ref as orf
from tests import seam_meshes as sm
from tests import shells_ref as sr


def restated(mesh, geometry=False):
    """(render arrays, edges, shells) of a mesh from its arrays"""
    I, vs, tf, nf = sm.arrays_of(mesh)
    e = er.build(I, vs)
    return (I, vs, tf, nf), e, sr.build(I, vs, tf, nf, e, mesh[0] if geometry else None)


# ---- orient: 4096-triangle tiles (kCoverTris)
@pytest.mark.parametrize("name", sorted(sm.FANS))
def test_fan_on_seam(name):
    degree, lead, tile = sm.FANS[name]
    mesh = sm.fan_on_seam(degree, lead, tile)
    (I, vs, tf, nf), e, _ = restated(mesh)
    one_face, fan, joining = sm.fan_on_seam_counts(I, vs, tf, e, tile)
    assert one_face and joining == 0 and fan.tolist() == list(range(tile - lead, tile - lead + degree - 2))
    o = orf.of_arrays(*mesh, majority=True, outward=True)
    assert len(set(o["tri_patch"][fan].tolist())) == 1 and o["tri_patch"][fan[0]] == 1
    # the fan is a patch of its own: one face, every side open; the strip before it and each fin are the others
    assert o["patch_counts"][1].tolist() == [degree - 2, 1, 0, 0, 0, 3 * (degree - 2), 1, 0]
    assert o["summary"] == (2 + 2 * (degree - 3),) * 2 + (0, 0, 0, 0)
    if degree == 5:
        assert o["patch_counts"][1].tolist() == [3, 1, 0, 0, 0, 9, 1, 0]


@pytest.mark.parametrize("name", sorted(sm.TWO_TILES))
def test_one_patch_over_two_tiles(name):
    make, (patches, orientable, inverted) = sm.TWO_TILES[name]
    mesh = make()
    (I, vs, tf, nf), e, _ = restated(mesh)
    pairs, n_edge = sm.orient_pairs(I, vs, tf, e)
    assert sm.COVER_TRIS < len(I) <= 2 * sm.COVER_TRIS and sm.leaving(pairs, sm.COVER_TRIS) >= 2   # the patch closes round both tiles
    o = orf.of_arrays(*mesh)
    assert o["summary"][:2] == (patches, orientable) and o["summary"][3] == inverted
    if name == "moebius":
        assert o["summary"] == (1, 0, 0, 0, 1, 1)
    if name == "klein":
        assert o["summary"] == (1, 0, 0, 0, 48, 48)
    if name == "torus_quads_turned":
        assert len(pairs) - n_edge == 48 * 48 and (np.asarray(mesh[1]) == 4).all()      # a same-face relation per quad beside the edges'
    if orientable:
        assert o["summary"][5] == 0 and o["summary"][4] > 0                            # the turns are against edges, and all can go


@pytest.mark.parametrize("reverse", [False, True], ids=["ascending", "reversed"])
@pytest.mark.parametrize("ntri", sm.ORIENT_STRIPS)
def test_orient_strips(ntri, reverse):
    mesh, flags = sm.turned_strip(ntri, reverse)
    (I, vs, tf, nf), e, _ = restated(mesh)
    pairs, _ = sm.orient_pairs(I, vs, tf, e)
    assert len(I) == ntri and sm.leaving(pairs, sm.COVER_TRIS) == (ntri - 1) // sm.COVER_TRIS
    o = orf.of_arrays(*mesh, majority=True)
    assert o["summary"][:2] == (1, 1) and o["summary"][2] == flags.sum() and np.array_equal(o["face_flip"] != 0, flags)


# ---- shells: 8192-triangle tiles (kHookTris), 32 partials a lane (kSegMax), 256 a tile of the workgroup's sum
@pytest.mark.parametrize("reverse", [False, True], ids=["ascending", "reversed"])
@pytest.mark.parametrize("ntri", sm.SHELL_STRIPS + [sm.LONG_STRIP])
def test_shell_strips(ntri, reverse):
    _, e, s = restated(sm.strip(ntri, reverse))
    entries, span = sm.chunk_entries(s["tri_shell"])
    want = -(-ntri // sm.CHUNK)
    assert entries.tolist() == [want] and span.tolist() == [want] and sm.leaving(sm.shell_pairs(e), sm.HOOK_TRIS) == (ntri - 1) // sm.HOOK_TRIS
    assert {8192: 32, 8193: 33, 65795: 258}.get(ntri, want) == want
    assert s["summary"] == (1, 0, 0, 0, 1, ntri)


def test_shuffled_torus():
    mesh = sm.shuffled_torus()
    (I, vs, tf, nf), e, s = restated(mesh)
    sp, (op, _) = sm.shell_pairs(e), sm.orient_pairs(I, vs, tf, e)
    assert len(I) == 24576 and len(sp) == len(op) == 36864
    assert sm.leaving(sp, sm.HOOK_TRIS) == 24477 and sm.leaving(op, sm.COVER_TRIS) == 30614      # as counted when the case was designed
    assert 2 * sm.leaving(sp, sm.HOOK_TRIS) >= len(sp) and 2 * sm.leaving(op, sm.COVER_TRIS) >= len(op)
    assert s["summary"] == (1, 1, 0, 0, 0, 24576) and sr.genus(s["shell_counts"][0]) == 1
    assert orf.of_arrays(*mesh)["summary"] == (1, 1, 0, 0, 0, 0)


def test_alternating_blocks():
    _, _, s = restated(sm.alternating_blocks())
    entries, span = sm.chunk_entries(s["tri_shell"])
    assert entries.tolist() == [40, 40] and span.tolist() == [79, 79] and (entries > sm.SEG_MAX).all() and (span > entries).all()
    assert s["summary"] == (2, 0, 0, 0, 2, 40 * 256) and s["shell_first"].tolist() == [0, 256]


def test_confetti():
    mesh = sm.confetti()
    _, _, s = restated(mesh)
    o = orf.of_arrays(*mesh, majority=True, outward=True)
    n = len(mesh[1])
    assert n == 3000 > sm.SCAN_BLOCK > sm.LABEL_BLOCK
    assert s["summary"] == (n, 0, 0, 0, n, 1) and o["summary"] == (n, n, 0, 0, 0, 0)
    assert sm.labels_per_wavefront(s["tri_shell"]) == sm.labels_per_wavefront(o["tri_patch"]) == sm.WAVE


def test_interleaved_strips():
    mesh, flags = orf.random_turns(sm.interleaved_strips())
    _, _, s = restated(mesh)
    o = orf.of_arrays(*mesh, majority=True, outward=True)
    assert s["summary"][0] == o["summary"][0] == o["summary"][1] == sm.WAVE and s["summary"][5] == 48
    assert sm.labels_per_wavefront(s["tri_shell"]) == sm.labels_per_wavefront(o["tri_patch"]) == sm.WAVE
    entries, span = sm.chunk_entries(s["tri_shell"])
    assert (entries == len(flags) // sm.CHUNK).all() and (span == entries).all()   # every label in every chunk
    assert 0 < o["summary"][2] <= flags.sum()                                        # majority: the smaller side of every strip


# ---- edges and normals: 32-element segments (kEdgeSegMax, kNrmSegMax), a 256-thread sort
@pytest.mark.parametrize("pages", sm.BOOK_PAGES)
def test_books(pages):
    _, e, s = restated(sm.book(pages))
    lens = sm.segment_lengths(e)
    assert lens.max() == pages and (lens == pages).sum() == 1 and (lens > sm.SEG_MAX).sum() == (1 if pages > sm.SEG_MAX else 0)
    assert e["summary"][3] == 1 and s["summary"][:3] == (2, 0, 1)


def test_shelf():
    _, e, s = restated(sm.shelf())
    lens = sm.segment_lengths(e)
    assert lens.max() == 33 and (lens > sm.SEG_MAX).sum() == (lens == 33).sum() == 20
    assert e["summary"][3] == 20 and s["summary"][:3] == (40, 0, 20)


def test_hub_discs():
    mesh = sm.hub_discs()
    (I, vs, tf, nf), e, s = restated(mesh)
    corners = sm.corners_per_vertex(I, vs, len(mesh[0]))
    assert len(I) == 2694 and sorted(corners[corners > 8].tolist()) == sm.HUB_VALENCES    # the centres; no other vertex comes near
    assert (corners > sm.SEG_MAX).sum() == 5 and (corners > sm.SORT_BLOCK).sum() == 1
    assert s["summary"][0] == 7 and s["shell_counts"][:, 4].tolist() == sm.HUB_VALENCES   # seven discs, each rim as long as its valence
