"""Render-ready buffers (include/harry_amd.h: hry_render_build), the parts that need no GPU: the entry points exist and refuse
null arguments, and the tests' restatement of the unweld (tests/render_ref.py) partitions the corners of every OBJ golden exactly as
the `f v/vt/vn` tuples of the file do -- which pins the GPU test's expected values to the files themselves."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

from harry_amd import _native as nat
from harry_amd import codec as hc
from tests import render_ref as rr
from tests import util

OBJ = os.path.join(util.ROOT, "tests", "golden", "obj")
OBJ_FILES = sorted(p for p in glob.glob(os.path.join(OBJ, "*.obj")) if ".dec." not in p)   # (*.dec.obj: the reference writer's outputs)


def test_render_symbols_exported():
    L = nat.load()
    for name in ("build", "nverts", "ntris", "get", "copy", "stat", "free"):
        assert hasattr(L, "hry_render_" + name), name


def test_render_null_arguments():
    L = nat.load()
    r = C.c_void_p(1)
    assert L.hry_render_build(None, None, C.byref(r)) == nat.E_ARG
    assert not r.value
    rows, width, typ = C.c_uint64(7), C.c_int(), C.c_int()
    assert L.hry_render_get(None, b"indices", None, C.byref(rows), C.byref(width), C.byref(typ)) == nat.E_ARG
    assert L.hry_render_copy(None, None, b"indices", None, 0) == nat.E_ARG
    assert L.hry_render_stat(None, None, None) == nat.E_ARG
    assert L.hry_render_nverts(None) == 0 and L.hry_render_ntris(None) == 0
    L.hry_render_free(None)


def obj_corner_tuples(text: bytes):
    """(v, vt, vn) of every corner of every `f` line, 0-based (negative indices count back from the elements read so far)"""
    counts = {"v": 0, "vt": 0, "vn": 0}
    out = []
    for line in text.decode().splitlines():
        tok = line.split()
        if not tok:
            continue
        if tok[0] in counts:
            counts[tok[0]] += 1
        elif tok[0] == "f":
            for corner in tok[1:]:
                parts = (corner.split("/") + ["", ""])[:3]
                t = []
                for kind, p in zip(("v", "vt", "vn"), parts):
                    if p == "":
                        t.append(rr.NONE)
                    else:
                        i = int(p)
                        t.append(i - 1 if i > 0 else counts[kind] + i)
                out.append(t)
    return np.array(out, np.int64).reshape(-1, 3)


@pytest.mark.parametrize("path", OBJ_FILES, ids=[os.path.basename(p) for p in OBJ_FILES])
def test_unweld_restatement_matches_obj_corners(path):
    with open(path, "rb") as f:
        text = f.read()
    mesh = hc.Mesh.from_obj(text, OBJ)
    tuples = obj_corner_tuples(text)
    assert len(tuples) == mesh.ne
    keys = rr.corner_keys(mesh)
    assert np.array_equal(keys[:, 0], tuples[:, 0])
    got, got_first = rr.first_occurrence(keys)
    want, want_first = rr.first_occurrence(tuples)
    assert np.array_equal(got, want) and np.array_equal(got_first, want_first)
    cmap, vsrc, csrc = rr.vertex_map(mesh)
    if rr.unwelded(mesh):
        assert np.array_equal(cmap, want) and np.array_equal(csrc, want_first) and np.array_equal(vsrc, tuples[want_first, 0])
    idx, tri_face = rr.fan(mesh.face_offsets(), cmap)
    assert len(tri_face) == mesh.ntri
