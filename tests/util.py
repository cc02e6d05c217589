"""Shared helpers for the test-suite (CPU side)."""
from __future__ import annotations

import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_BIN = os.path.join(ROOT, "oracle", "_ref", "harry_ref")


def _int_big_cases():
    from harry_amd import meshgen as mg
    t5250 = lambda: mg.torus(70, 75, seed=5)
    return {
        "int_full_5250": lambda: mg.with_integer_props(t5250(), values="full"),
        "int_edges_mixed": lambda: mg.with_integer_props(mg.with_nonmanifold(mg.torus(50, 56, polys="mixed", seed=6), 20, 8), values="edges"),
        # more vertices than the 16 384 entries of k_unpredict3's ring, which lossless uchar / ushort ride: the smallest torus past one wrap
        "int_full_17161": lambda: mg.with_integer_props(mg.torus(131, 131), values="full"),
        "int_bytefirst_5250": lambda: mg.with_integer_props(t5250(), values="full", byte_first=True),
        "int_face_5250": lambda: mg.with_integer_props(t5250(), values="full", face=True),
    }


# integer attributes of every PLY type on meshes too large to commit: name -> generator; the reference's answers (size and hash
# of its lossless stream) are in tests/golden/manifest.json under "big" (tests/golden/make_golden.py)
INT_BIG_CASES = _int_big_cases()


def flags_to_quant(flags):
    """Emulate the reference CLI's -l/-a/-q/-c state machine (main.cc:47-71): returns (triples, clear)."""
    cur_l, cur_a, out, clear = None, -1, [], False
    it = iter(flags)
    for f in it:
        if f.startswith("-l") and f != "-l":
            cur_l = int(f[2:])
        elif f == "-l":
            cur_l = int(next(it))
        elif f.startswith("-a") and f != "-a":
            cur_a = int(f[2:])
        elif f == "-a":
            cur_a = int(next(it))
        elif f.startswith("-q") and f != "-q":
            out.append((cur_l, cur_a, int(f[2:])))
            cur_a = -1
        elif f == "-q":
            out.append((cur_l, cur_a, int(next(it))))
            cur_a = -1
        elif f == "-c":
            clear = True
        else:
            raise ValueError(f)
    return out, clear


def parse_ref_decoded_ply(data: bytes, vstride: int, fstride: int):
    """Parse a BINARY PLY written by the reference's ply writer (formats/ply/writer.cc:106-192).

    The writer declares quantised components with their storage type but dumps the whole original-width
    record (writer.cc:72-75), so records are sliced with the strides of the ORIGINAL
    types (supplied by the caller) instead of trusting the header.
    Returns (vertex records u8[nv, vstride], degrees, flat indices, face records u8[nf, fstride]).
    """
    end = data.index(b"end_header\n") + len(b"end_header\n")
    hdr = data[:end].decode().split("\n")
    assert "binary_little_endian" in hdr[1]
    nv = nf = None
    for line in hdr:
        if line.startswith("element vertex"):
            nv = int(line.split()[2])
        if line.startswith("element face"):
            nf = int(line.split()[2])
    body = np.frombuffer(data, dtype=np.uint8, offset=end)
    vrec = body[: nv * vstride].reshape(nv, vstride)
    p = nv * vstride
    degs = np.zeros(nf, np.uint8)
    idx = []
    frec = np.zeros((nf, fstride), np.uint8)
    raw = body[p:].tobytes()
    q = 0
    for f in range(nf):
        d = raw[q]
        degs[f] = d
        q += 1
        idx.append(np.frombuffer(raw, dtype="<u4", count=d, offset=q))
        q += 4 * d
        frec[f] = np.frombuffer(raw, dtype=np.uint8, count=fstride, offset=q)
        q += fstride
    assert q == len(raw), (q, len(raw))
    return vrec, degs, (np.concatenate(idx) if idx else np.zeros(0, "<u4")), frec


def canonical_faces(vrec: np.ndarray, degs: np.ndarray, idx: np.ndarray):
    """Order-independent description of a mesh: sorted list of faces, each a tuple of vertex records rotated
    to start at its smallest record (the codec permutes vertices and faces, SURVEY finding 0-4)."""
    out = []
    off = 0
    keys = [bytes(r) for r in vrec]
    for d in degs:
        d = int(d)
        vs = [keys[int(i)] for i in idx[off:off + d]]
        off += d
        k = min(range(d), key=lambda j: (vs[j], vs[(j + 1) % d]))
        out.append(tuple(vs[k:] + vs[:k]))
    out.sort()
    return out


def random_ply_case(seed: int):
    """Seeded random PLY input beyond the committed fixtures: (PLY bytes, the two flag sets it is encoded with).  The reference's
    answers on these inputs are recorded in tests/golden/random.json (tests/golden/make_golden_random.py)."""
    from harry_amd import meshgen as mg
    rng = np.random.default_rng(100 + seed)
    nu, nv = int(rng.integers(6, 40)), int(rng.integers(3, 20)) * 2
    polys = ["tri", "quad", "mixed"][seed % 3]
    m = mg.torus(nu, nv, seed=seed, polys=polys, normals=bool(seed & 1))
    if seed == 3:
        m = mg.with_nonmanifold(mg.concat([m, mg.torus(7, 8, seed=9, polys=polys, normals=bool(seed & 1), center=(5, 0, 0))]), 4, 3)
    return m.to_ply(), [[], ["-l1", f"-q{int(rng.integers(2, 17))}"]]


def random_scene_cases():
    """Seeded random OBJ scenes and PLY meshes beyond the committed fixtures: yields (file name, source bytes, flags).  The
    reference's answers on these inputs are recorded in tests/golden/random.json (tests/golden/make_golden_random.py)."""
    from harry_amd import meshgen as mg
    from harry_amd import objgen as og
    rng = np.random.default_rng(23)
    for it in range(16):
        polys = ["tri", "quad", "mixed"][int(rng.integers(0, 3))]
        base = [lambda: mg.torus(int(rng.integers(5, 22)), int(rng.integers(5, 22)), polys=polys, seed=int(rng.integers(1, 99))),
                lambda: mg.icosphere(int(rng.integers(1, 4))),
                lambda: mg.with_nonmanifold(mg.multi_component(int(rng.integers(2, 5)), 8, 9, polys=polys), int(rng.integers(1, 5)), int(rng.integers(1, 3)), seed=int(rng.integers(1, 99)))][int(rng.integers(0, 3))]()
        flags = []
        if it % 2 == 0:
            sc = og.scene(base, normals=[None, "smooth", "flat"][int(rng.integers(0, 3))], tex=[None, "atlas", "corner"][int(rng.integers(0, 3))],
                          charts=int(rng.integers(1, 7)), colors=[None, "all", "some"][int(rng.integers(0, 3))], tex3=bool(rng.integers(0, 2)),
                          interleave=bool(rng.integers(0, 2)), negative=bool(rng.integers(0, 2)), seed=int(rng.integers(1, 99)))
            name, src = f"s{it}.obj", sc.obj
            if rng.integers(0, 2):
                flags = ["-l0", f"-q{int(rng.integers(6, 17))}"]
        else:
            name, src = f"s{it}.ply", base.to_ply(["binary_little_endian", "binary_big_endian", "ascii"][int(rng.integers(0, 3))])
            if rng.integers(0, 2):
                flags = ["-l1", f"-q{int(rng.integers(6, 17))}"]
        yield name, src, flags


def oracle_shard(shard, whole_oracle):
    """The CPU oracle's copy of a product shard (harry_amd.codec.Mesh from ShardPlan.extract): same elements in the same
    order (through PLY), the whole mesh's bounds and polygon degrees, the shard's seeds and runs."""
    from oracle import oracle_py as op
    if shard.nf == 0:
        o = whole_oracle.clone()   # formats only; no face is coded
        raise ValueError("empty shard: nothing to restate")
    o = op.Mesh.from_ply(shard.to_ply())
    for l in (0, 1):
        if whole_oracle.list_fmt(l):
            o.set_bounds(l, bytes(whole_oracle.list_min(l)), bytes(whole_oracle.list_max(l)))
    o.set_degrees(whole_oracle.degrees())
    o.set_shard(whole_oracle.nv, whole_oracle.nf, whole_oracle.ne, shard.shard_elements(2), shard.runs())
    return o


# ---- shared by the tests of the builds behind a render build (test_gpu_edges / _shells / _orient / _seams)
def xyz(pos):
    """vertex records x y z (f32) from an [n, 3] array"""
    pos = np.asarray(pos, np.float32)
    v = np.zeros(len(pos), np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4")]))
    v["x"], v["y"], v["z"] = pos[:, 0], pos[:, 1], pos[:, 2]
    return v


def xyz_mesh(pos, tris):
    """a triangle mesh from positions [n, 3] and triangles [T, 3]"""
    from harry_amd import codec as hc
    tris = np.asarray(tris, np.uint32).reshape(-1, 3)
    return hc.Mesh.from_arrays(xyz(pos), np.full(len(tris), 3, np.uint8), tris.reshape(-1))


def position_list(mesh):
    ls = [l for l in range(mesh.nlists) if mesh.list_target(l) == 1 and len(mesh.list_fmt(l)) >= 3]
    assert len(ls) == 1
    return ls[0]


def same_bytes(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
