"""The self-intersection build over the hierarchy (hry_intersections_build) on configs[1] (1 002 528 triangles, -l1 -q14, chunked
container), resident after a decode, through Codec.bvh and Bvh.intersections: the torus alone, where no pair is expected, and the
torus beside its copy moved by (0.3, 0.1, 0.05), which passes through it.  Prints ONE JSON line; per case ("alone_", "shifted_"):
  build_ms           the kernels of hry_bvh_build on that mesh (HIP events, hry_bvh_stat), rebuilt in every round like the query
  query_ms           the kernels of hry_intersections_build, both stretches (hry_intersections_stat); query_over_build: their ratio
  mleaves            leaves / query time; box_tests: box tests of the walk per leaf
  candidates / tested / pairs / triangles_hit   C, N, P, H of the summary
  checked / mismatches   the rows of pairs of so many triangles against a float64 torch brute force: their leaf box against every
                     leaf's box, then the contract's clauses on what overlaps; the triangles whose set of partners or whose shared
                     counts differ
Warm-up runs first, then medians over the repeats, with the smallest and largest run beside them ("_range").  No threshold is set
on any of these."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from harry_amd import codec as hc  # noqa: E402
from harry_amd import meshgen as mg  # noqa: E402


def brute_force(torch, buffers, leaves, chunk=64):
    """the contract for the leaves `leaves` against every leaf, in float64, every operation a kernel of its own -> (keys int64: t << 32 |
    s of the pairs found, ascending; their shared counts)"""
    f64 = torch.float64
    box, P, tri_of = buffers["leaf_box"], buffers["leaf_positions"].to(f64).reshape(-1, 3, 3), buffers["leaf_tri"].to(torch.int64)
    dot = lambda a, b: (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]
    cross = lambda a, b: torch.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                                      a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], dim=-1)
    ii, jj = [], []
    for at in range(0, len(leaves), chunk):
        mine = box[leaves[at:at + chunk]][:, None, :]
        meet = ((mine[..., :3] <= box[None, :, 3:]) & (box[None, :, :3] <= mine[..., 3:])).all(dim=-1)
        a, b = torch.nonzero(meet, as_tuple=True)
        ii.append(leaves[at:at + chunk][a])
        jj.append(b)
    i, j = torch.cat(ii), torch.cat(jj)
    keep = i != j
    i, j = i[keep], j[keep]
    A, B = P[i], P[j]

    def proper(X):
        n = cross(X[:, 1] - X[:, 0], X[:, 2] - X[:, 0])
        return dot(n, n) > 0

    def meets(a, b, tri):
        d = b - a
        e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
        p = cross(d, e2)
        det = dot(e1, p)
        s = a - tri[:, 0]
        q = cross(s, e1)
        u, v, tt = dot(s, p) / det, dot(d, q) / det, dot(e2, q) / det
        return torch.isfinite(det) & (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (0 <= tt) & (tt <= 1)

    same = (A[:, :, None, :] == B[:, None, :, :]).all(dim=3)
    share = same.any(dim=2).sum(dim=1)
    ka, kb = same.any(dim=2).to(torch.int8).argmax(dim=1), same.any(dim=1).to(torch.int8).argmax(dim=1)
    hit = torch.zeros(len(i), dtype=torch.bool, device=i.device)
    for k in range(3):
        hit |= ((share == 0) | ((share == 1) & ((ka + 1) % 3 == k))) & meets(A[:, k], A[:, (k + 1) % 3], B)
        hit |= ((share == 0) | ((share == 1) & ((kb + 1) % 3 == k))) & meets(B[:, k], B[:, (k + 1) % 3], A)
    hit &= proper(A) & proper(B) & (share <= 1)
    t, s = tri_of[i][hit], tri_of[j][hit]
    keys = (torch.minimum(t, s) << 32) | torch.maximum(t, s)
    keys, where = torch.unique(keys, return_inverse=True)   # (a pair of two sampled leaves is met from both)
    shared = torch.zeros(len(keys), dtype=torch.int64, device=keys.device)
    shared[where] = share[hit]
    return keys, shared


def xyz(pos):
    v = np.zeros(len(pos), np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4")]))
    v["x"], v["y"], v["z"] = pos[:, 0], pos[:, 1], pos[:, 2]
    return v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--side", type=int, default=708, help="torus grid side; 708 -> 1 002 528 triangles (configs[1])")
    ap.add_argument("--check", type=int, default=4096, help="triangles whose rows of pairs go through the brute force")
    args = ap.parse_args()
    import torch
    torch.cuda.init()   # torch holds the device before the codec starts
    cx = hc.Codec(0)
    try:
        g = mg.torus(args.side, args.side, seed=2, sigma=1e-4)
        m = hc.Mesh.from_arrays(g.verts, g.degrees, g.indices)
        cx.requant(m, [(1, -1, 14)])
        alone = cx.read_hry(cx.write_hry(m, profile=hc.PROFILE_CHUNKED))
        pos, tri = np.ascontiguousarray(cx.position_rows(alone), np.float32), cx.render_numpy(alone)["indices"].astype(np.uint32)
        both = np.concatenate([pos, (pos + np.float32([0.3, 0.1, 0.05])).astype(np.float32)])
        shifted = hc.Mesh.from_arrays(xyz(both), np.full(2 * len(tri), 3, np.uint8), np.concatenate([tri, tri + np.uint32(len(pos))]).reshape(-1))
        res = {"ntris": int(g.ntri)}
        for name, mesh in (("alone", alone), ("shifted", shifted)):
            b, build = None, []
            for i in range(args.warmup + args.repeats):   # the build timed like the query: rebuilt every round
                if b is not None:
                    b.close()
                b = cx.bvh(mesh)
                if i >= args.warmup:
                    build.append(cx.bvh_stat()["device_ms"])
            build_ms, leaves = statistics.median(build), b.count()
            ms = []
            for i in range(args.warmup + args.repeats):
                x = b.intersections()
                if i >= args.warmup:
                    ms.append(x.device_ms)
                if i + 1 < args.warmup + args.repeats:
                    x.close()
            med = statistics.median(ms)
            res.update({f"{name}_leaves": leaves, f"{name}_build_ms": build_ms, f"{name}_build_ms_range": [min(build), max(build)], f"{name}_query_ms": med,
                        f"{name}_query_ms_range": [min(ms), max(ms)], f"{name}_query_over_build": med / build_ms, f"{name}_mleaves": leaves / med / 1e3, f"{name}_box_tests": x.box_tests / max(leaves, 1),
                        f"{name}_candidates": x.candidates, f"{name}_tested": x.tested, f"{name}_pairs": x.pairs, f"{name}_triangles_hit": x.triangles_hit})
            n = min(args.check, leaves)
            if n:
                buffers, got = b.buffers(), x.buffers()
                pick = torch.arange(n, device="cuda") * (leaves // n)
                keys, shared = brute_force(torch, buffers, pick)
                sampled = buffers["leaf_tri"].to(torch.int64)[pick]
                t, s = got["pairs"][:, 0].to(torch.int64), got["pairs"][:, 1].to(torch.int64)
                mine = torch.isin(t, sampled) | torch.isin(s, sampled)
                dev_keys, dev_shared = ((t << 32) | s)[mine], got["pair_shared"].to(torch.int64)[mine]   # (ascending already)
                if len(dev_keys) == len(keys) and bool((dev_keys == keys).all()) and bool((dev_shared == shared).all()):
                    wrong = 0
                else:   # the sampled triangles in a pair only one side has, or with another shared count
                    a = set(zip(dev_keys.tolist(), dev_shared.tolist()))
                    c = set(zip(keys.tolist(), shared.tolist()))
                    ids = set(sampled.tolist())
                    wrong = len({end for k, _ in a ^ c for end in (k >> 32, k & 0xffffffff) if end in ids})
                res.update({f"{name}_checked": n, f"{name}_checked_pairs": len(keys), f"{name}_mismatches": wrong})
            x.close()
            b.close()
        print(json.dumps(res))
    finally:
        cx.close()


if __name__ == "__main__":
    main()
