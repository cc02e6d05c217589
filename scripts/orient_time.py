"""Consistent winding per patch (hry_orient_build) through Codec.orient on BASELINE configs[1] -- 1 002 528 triangles, one closed
patch -- with 30 % of its faces turned (fixed seed), resident after a decode (-l1 -q14, chunked container), beside the shells build
of the same mesh and a host baseline.  Prints ONE JSON line:
  device_ms_relative / _majority / _outward  the orient kernels' device_ms (HIP events, hry_orient_stat): no flag, HRY_ORIENT_MAJORITY,
                                             HRY_ORIENT_MAJORITY | HRY_ORIENT_OUTWARD
  wall_ms_*                                  Codec.orient as a caller sees it: render, edges and orient builds and the copies into torch tensors
  shells_device_ms / shells_geometry_device_ms   hry_shells_build of the same mesh, without and with HRY_SHELLS_GEOMETRY: the same inputs, one
                                             union-find over T nodes where the orientation has 2 T
  scipy_ms                                   where scipy imports: a parity breadth-first pass on the host over Codec.edges' tri_neighbours,
                                             including the copy down of indices / vertex_source / tri_neighbours: scipy's
                                             breadth_first_order for the tree, whether a triangle is against its predecessor from
                                             the two directed sides, the parity along the tree by pointer doubling in numpy
Each build follows a fresh decode; warm-up runs first, then medians over the repeats, with the smallest and largest run beside them
("_range").  The baseline gives the relative flips of one patch only: no patches, counts, orientability or measures."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from harry_amd import codec as hc  # noqa: E402
from harry_amd import meshgen as mg  # noqa: E402


def median_of(f, args):
    dev, wall = [], []
    for i in range(args.warmup + args.repeats):
        d, w = f()
        if i >= args.warmup:
            dev.append(d)
            wall.append(w)
    return statistics.median(dev), [min(dev), max(dev)], statistics.median(wall), [min(wall), max(wall)]


def host_parity(torch, r, e):
    """relative flips of every triangle of the patch of triangle 0 (numpy bool [T]), and how many triangles it reached"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import breadth_first_order
    I = r["indices"].cpu().numpy().astype(np.int64)
    vs = r["vertex_source"].cpu().numpy().astype(np.int64)
    tn = e["tri_neighbours"].cpu().numpy().astype(np.int64)
    T = len(I)
    t, k = np.nonzero(tn >= 0)
    g = coo_matrix((np.ones(len(t), np.int8), (t, tn[t, k])), shape=(T, T)).tocsr()
    order, pred = breadth_first_order(g, 0, directed=False)
    node = order[1:]
    p = pred[node]
    frm, to = vs[I], vs[I[:, [1, 2, 0]]]
    side = np.argmax(tn[node] == p[:, None], axis=1)                   # the side of `node` that faces its predecessor
    a, b = frm[node, side], to[node, side]
    against = ((frm[p] == a[:, None]) & (to[p] == b[:, None])).any(axis=1)   # the predecessor runs a -> b too
    par = np.arange(T)
    w = np.zeros(T, bool)
    par[node], w[node] = p, against
    while True:                                                        # parity along the tree, pointer doubling
        nxt = par[par]
        if np.array_equal(nxt, par):
            return w, len(order)
        w ^= w[par]
        par = nxt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--fraction", type=float, default=0.3)
    args = ap.parse_args()
    import torch
    torch.cuda.init()   # torch holds the device before the codec starts
    cx = hc.Codec(0)
    try:
        g = mg.torus(708, 708, seed=2, sigma=1e-4)
        tris = g.indices.reshape(-1, 3).copy()
        turn = np.random.default_rng(11).random(len(tris)) < args.fraction
        tris[turn] = tris[turn][:, [0, 2, 1]]
        m = hc.Mesh.from_arrays(g.verts, g.degrees, tris.reshape(-1))
        cx.requant(m, [(1, -1, 14)])
        blob = cx.write_hry(m, profile=hc.PROFILE_CHUNKED)
        T, k = len(tris), int(turn.sum())
        res = {"ntris": T, "turned": k}

        def timed(build, stat):
            def f():
                mesh = cx.read_hry(blob)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                build(mesh)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                assert stat()["uploaded_bytes"] == 0
                return stat()["device_ms"], (t1 - t0) * 1e3
            return f

        for key, kw in (("relative", {}), ("majority", {"majority": True}), ("outward", {"majority": True, "outward": True})):
            d, dr, w, wr = median_of(timed(lambda mesh: cx.orient(mesh, **kw), cx.orient_stat), args)
            res.update({"device_ms_" + key: d, "device_ms_" + key + "_range": dr, "wall_ms_" + key: w, "wall_ms_" + key + "_range": wr})
            st = cx.orient_stat()
            assert st["patches"] == st["orientable"] == 1 and st["remaining"] == 0 and st["against"] > 0
            if key == "majority":
                assert st["flipped"] == min(k, T - k)
        res.update({x: st[x] for x in ("patches", "orientable", "flipped", "inverted", "against", "remaining")})
        for key, geometry in (("shells_device_ms", False), ("shells_geometry_device_ms", True)):
            d, dr, _, _ = median_of(timed(lambda mesh: cx.shells(mesh, geometry=geometry), cx.shells_stat), args)
            res[key], res[key + "_range"] = d, dr

        try:
            import scipy  # noqa: F401
        except ImportError:
            print(json.dumps(res))
            return
        mesh = cx.read_hry(blob)
        r, e, want = cx.render(mesh), cx.edges(mesh), cx.orient(mesh)
        ms = []
        for i in range(args.warmup + args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            flips, reached = host_parity(torch, r, e)
            t1 = time.perf_counter()
            if i >= args.warmup:
                ms.append((t1 - t0) * 1e3)
        assert reached == T and np.array_equal(flips, want["tri_flip"].cpu().numpy() != 0)   # the same relative flips
        res["scipy_ms"], res["scipy_ms_range"] = statistics.median(ms), [min(ms), max(ms)]
        print(json.dumps(res))
    finally:
        cx.close()


if __name__ == "__main__":
    main()
