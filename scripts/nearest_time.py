"""The closest-point query over the hierarchy (hry_bvh_nearest) on configs[1] (1 002 528 triangles, -l1 -q14, chunked container),
resident after a decode, through Codec.bvh and Bvh.nearest.  Prints ONE JSON line:
  build_device_ms    the build's kernels (HIP events, hry_bvh_stat)
  random_ms / random_mpoints     1 M random points about the scene (its box grown by a half), in no order: the query's kernel, and
                     points / time
  decode_ms / decode_mpoints     the vertices of a -q12 decode of the same mesh against the -q14 surface: points close to it, in
                     the decoder's order
  random_bounds / decode_bounds  box bounds evaluated per point; decode_max / decode_rms: the deviation those vertices have
  checked / mismatches   a subset of the random points against a chunked float64 torch brute force of the contract's rule (every
                     triangle's candidates, the clamp by its leaf box's bound): the points whose triangle, d2, uv or point differ
                     in any bit
Warm-up runs first, then medians over the repeats, with the smallest and largest run beside them ("_range").  No threshold is set
on any of these."""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from harry_amd import codec as hc  # noqa: E402
from harry_amd import meshgen as mg  # noqa: E402


def brute_force(torch, buffers, q, chunk=4):
    """the contract's rule for every (point, leaf) in float64, every operation a kernel of its own -> (tri int32, d2 float64, uv, point
    float32)"""
    f64 = torch.float64
    box, P, tri_of = buffers["leaf_box"].to(f64), buffers["leaf_positions"].to(f64).reshape(-1, 3, 3), buffers["leaf_tri"].to(torch.int64)
    lo, hi, inf = box[None, :, :3], box[None, :, 3:], float("inf")
    dot = lambda a, b: (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]
    cross = lambda a, b: torch.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                                      a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], dim=-1)
    P0, P1, P2 = P[None, :, 0], P[None, :, 1], P[None, :, 2]
    e1, e2 = P1 - P0, P2 - P0
    n = cross(e1, e2)
    nn = dot(n, n)
    safe = torch.where(nn > 0, nn, 1.0)

    def segment(A, B, Q):
        d = B - A
        l = dot(d, d)
        s = dot(Q - A, d) / torch.where(l == 0, 1.0, l)
        return torch.where(l == 0, 0.0, torch.where(s < 0, 0.0, torch.where(s > 1, 1.0, s)))

    out = [[], [], [], []]
    for at in range(0, len(q), chunk):
        Q = q[at:at + chunk].to(f64)[:, None, :]
        s = Q - P0
        u, v = dot(cross(s, e2), n) / safe, dot(cross(e1, s), n) / safe
        sb, sc, sd = segment(P0, P1, Q), segment(P1, P2, Q), segment(P2, P0, Q)
        zero = torch.zeros_like(sb)
        best, bu, bv, bc = torch.full_like(sb, inf), zero, zero, torch.zeros(sb.shape + (3,), dtype=f64, device=sb.device)
        for ok, cu, cv in (((nn > 0) & (u >= 0) & (v >= 0) & (u + v <= 1), u, v), (None, sb, zero), (None, 1.0 - sc, sc), (None, zero, 1.0 - sd)):
            c = P0 + (cu[..., None] * e1 + cv[..., None] * e2)
            d2 = dot(Q - c, Q - c)
            take = d2 < best if ok is None else ok & (d2 < best)
            best, bu, bv, bc = torch.where(take, d2, best), torch.where(take, cu, bu), torch.where(take, cv, bv), torch.where(take[..., None], c, bc)
        g = torch.clamp(torch.maximum(lo - Q, Q - hi), min=0.0)
        b2 = (g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + g[..., 2] * g[..., 2]
        dt = torch.where(b2 > best, b2, best)
        least = dt.amin(dim=1, keepdim=True)
        leaf = torch.where(dt == least, tri_of[None, :], 1 << 40).argmin(dim=1)
        k = torch.arange(len(leaf), device=leaf.device)
        out[0].append(tri_of[leaf].to(torch.int32))
        out[1].append(dt[k, leaf])
        out[2].append(torch.stack([bu[k, leaf], bv[k, leaf]], dim=1).to(torch.float32))
        out[3].append(bc[k, leaf].to(torch.float32))
    return [torch.cat(x) for x in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--side", type=int, default=708, help="torus grid side; 708 -> 1 002 528 triangles (configs[1])")
    ap.add_argument("--points", type=int, default=1 << 20, help="random points about the scene")
    ap.add_argument("--check", type=int, default=4096, help="random points that go through the brute force")
    args = ap.parse_args()
    import torch
    torch.cuda.init()   # torch holds the device before the codec starts
    cx = hc.Codec(0)
    try:
        g = mg.torus(args.side, args.side, seed=2, sigma=1e-4)

        def decoded(bits):
            m = hc.Mesh.from_arrays(g.verts, g.degrees, g.indices)
            cx.requant(m, [(1, -1, bits)])
            return cx.read_hry(cx.write_hry(m, profile=hc.PROFILE_CHUNKED))

        b = cx.bvh(decoded(14))
        st = cx.bvh_stat()
        buffers = b.buffers()
        scene = buffers["scene_box"][0]
        mid, half = (scene[:3] + scene[3:]) / 2, (scene[3:] - scene[:3]) / 2
        gen = torch.Generator(device="cuda").manual_seed(1)
        random = (mid + 1.5 * half * (2 * torch.rand(args.points, 3, device="cuda", generator=gen) - 1)).contiguous()
        coarse = torch.from_numpy(cx.position_rows(decoded(12)).copy()).cuda()
        res = {"ntris": int(g.ntri), "build_device_ms": st["device_ms"]}
        for name, pts in (("decode", coarse), ("random", random)):
            ms = []
            for i in range(args.warmup + args.repeats):
                got = b.nearest(pts)
                if i >= args.warmup:
                    ms.append(b.device_ms)
            res.update({f"{name}_points": len(pts), f"{name}_ms": statistics.median(ms), f"{name}_ms_range": [min(ms), max(ms)],
                        f"{name}_mpoints": len(pts) / statistics.median(ms) / 1e3, f"{name}_answered": b.answered, f"{name}_bounds": b.bound_tests / len(pts),
                        f"{name}_max": math.sqrt(b.max_d2)})
            if name == "decode":
                res["decode_rms"] = math.sqrt(float(got["d2"].sum()) / len(pts))
        n = min(args.check, len(random))
        if n:
            pick = torch.arange(n, device="cuda") * (len(random) // n)
            tri, d2, uv, point = brute_force(torch, buffers, random[pick])
            differ = (tri != got["tri"][pick]) | (d2.view(torch.int64) != got["d2"][pick].view(torch.int64)) | \
                     (uv.view(torch.int32) != got["uv"][pick].view(torch.int32)).any(dim=1) | (point.view(torch.int32) != got["point"][pick].view(torch.int32)).any(dim=1)
            res.update({"checked": n, "mismatches": int(differ.sum())})
        res.update({k: st[k] for k in hc.Bvh.SUMMARY})
        print(json.dumps(res))
        b.close()
    finally:
        cx.close()


if __name__ == "__main__":
    main()
