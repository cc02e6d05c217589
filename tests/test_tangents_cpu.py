"""What of the tangent frames needs no GPU: the entry points of hry_tangents_build (include/harry_amd.h), and the restatement of
its contract (tests/tangents_ref.py) against closed forms."""
import ctypes as C
import os
import re

import numpy as np

from harry_amd import _native as nat
from tests import tangents_ref as tr
from tests import util

HEADER = os.path.join(util.ROOT, "include", "harry_amd.h")
NAMES = ("build", "count", "get", "copy", "summary", "stat", "free")


def test_header_declares_and_library_exports():
    text = open(HEADER).read()
    L = nat.load()
    for name in NAMES:
        assert re.search(r"\bhry_tangents_%s\(" % name, text), name
        assert hasattr(L, "hry_tangents_" + name), name
    assert "typedef struct hry_tangents hry_tangents;" in text
    for flag, value in (("ANGLE_WEIGHTED", 1), ("STORED_NORMALS", 2), ("BITANGENTS", 4)):
        assert re.search(r"#define HRY_TANGENTS_%s\s+%du\b" % (flag, value), text), flag
        assert getattr(nat, "TANGENTS_" + flag) == value
    assert re.search(r"#define HRY_ABI_VERSION\s+6\b", text) and L.hry_abi_version() == 6


def test_null_arguments_without_a_device():
    L = nat.load()
    out = C.c_void_p(1)
    assert L.hry_tangents_build(None, None, None, 0, C.byref(out)) == nat.E_ARG and not out.value
    assert L.hry_tangents_build(None, None, None, 0, None) == nat.E_ARG
    assert L.hry_tangents_count(None) == 0
    s = (C.c_uint64 * 6)()
    assert L.hry_tangents_summary(None, s) == nat.E_ARG and L.hry_tangents_stat(None, None, None) == nat.E_ARG
    L.hry_tangents_free(None)


# ---- the restatement against closed forms
def flat_grid(n=5, m=4):
    j, i = np.meshgrid(np.arange(m), np.arange(n))
    pos = np.stack([i.ravel() / (n - 1), j.ravel() / (m - 1), np.zeros(n * m)], 1).astype(np.float32)
    a = (np.arange(n - 1)[:, None] * m + np.arange(m - 1)[None, :]).ravel()
    b, c, d = a + 1, a + m + 1, a + m
    # (counter-clockwise seen from +z)
    tris = np.stack([np.stack([a, c, b], 1), np.stack([a, d, c], 1)], 1).reshape(-1, 3)
    nrm = np.tile(np.float32([0, 0, 1]), (n * m, 1))
    return pos, nrm, tris


def rotated_uv(pos, flip_u=False):
    u, v = 0.8 * pos[:, 0] + 0.6 * pos[:, 1], -0.6 * pos[:, 0] + 0.8 * pos[:, 1]
    return np.stack([-u if flip_u else u, v], 1).astype(np.float32)


def test_flat_grid_gives_the_rotated_axis():
    pos, nrm, tris = flat_grid()
    for weights in ("area", "angle"):
        r = tr.tangents(pos, rotated_uv(pos), nrm, tris, weights)
        assert r["guard"].all() and r["summary"] == (len(pos), 0, 0, 0, 0)
        # P = u (0.8, 0.6) + v (-0.6, 0.8): the tangent is dP/du, the bitangent dP/dv = n x t, so w = +1.  The float32 uv carry 2^-24
        # of relative error, a direction from differences of them a few times that
        assert np.abs(r["tangents"][:, :3] - np.float32([0.8, 0.6, 0])).max() < 1e-5
        assert (r["tangents"][:, 3] == 1).all()
        assert np.abs(r["bitangents"] - np.float32([-0.6, 0.8, 0])).max() < 1e-5


def test_negating_u_flips_the_handedness():
    # u -> -u mirrors the map: every det changes sign and with it w, and nothing else about the frame changes: the bitangent dP/dv
    # keeps its value and the tangent, which points along growing u, is the exact negative
    pos, nrm, tris = flat_grid()
    for weights in ("area", "angle"):
        a = tr.tangents(pos, rotated_uv(pos), nrm, tris, weights)
        b = tr.tangents(pos, rotated_uv(pos, flip_u=True), nrm, tris, weights)
        assert (a["tangents"][:, 3] == 1).all() and (b["tangents"][:, 3] == -1).all()
        assert np.array_equal(b["tangents"][:, :3], -a["tangents"][:, :3])
        assert np.array_equal(b["bitangents"], a["bitangents"])   # (as values: a zero may change its sign)
        assert b["summary"] == (len(pos), 0, len(pos), 0, 0) and b["guard"].all()


def test_a_triangle_with_three_equal_uv_contributes_nothing():
    pos, nrm, tris = flat_grid()
    uv = rotated_uv(pos)
    whole = tr.tangents(pos, uv, nrm, tris)
    # a further triangle over three vertices of its own, all with one uv: the others' rows keep their bits, its vertices get no frame
    extra = np.float32([[2, 0, 0], [3, 0, 0], [2, 1, 0]])
    n = len(pos)
    r = tr.tangents(np.concatenate([pos, extra]), np.concatenate([uv, np.tile(np.float32([0.25, 0.5]), (3, 1))]), np.concatenate([nrm, nrm[:3]]),
                    np.concatenate([tris, [[n, n + 1, n + 2]]]))
    assert r["degenerate"].sum() == 1 and r["degenerate"][-1] and r["summary"] == (n, 3, 0, 0, 1)
    assert np.array_equal(r["tangents"][:n].view(np.uint32), whole["tangents"].view(np.uint32))
    assert not r["tangents"][n:].any() and not r["bitangents"][n:].any()
    # ... and where it shares its vertices with the grid it changes no bit there either
    shared = tr.tangents(pos, np.concatenate([uv[:-3], np.tile(np.float32([0.25, 0.5]), (3, 1))]), nrm, tris)
    again = tr.tangents(pos, np.concatenate([uv[:-3], np.tile(np.float32([0.25, 0.5]), (3, 1))]), nrm, np.concatenate([tris, [[n - 3, n - 2, n - 1]]]))
    assert again["summary"][4] == shared["summary"][4] + 1
    assert np.array_equal(again["tangents"].view(np.uint32), shared["tangents"].view(np.uint32))


def test_mixed_and_isolated():
    # a butterfly: two triangles that share vertex 0, the second with its uv wound the other way; vertex 5 is isolated
    pos = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0], [5, 5, 0]])
    uv = np.float32([[0, 0], [1, 0], [0, 1], [-1, 0], [0, 1], [0, 0]])
    nrm = np.tile(np.float32([0, 0, 1]), (6, 1))
    r = tr.tangents(pos, uv, nrm, [[0, 1, 2], [0, 3, 4]])
    assert r["mixed"].tolist() == [True, False, False, False, False, False]
    assert r["summary"][3] == 1 and r["summary"][1] >= 1 and not r["tangents"][5].any()
