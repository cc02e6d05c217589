"""The hierarchy over a render build and the cast over it (hry_bvh_build, hry_bvh_cast) on configs[1] (1 002 528 triangles, -l1
-q14, chunked container), resident after a decode, through Codec.bvh and Bvh.cast.  Prints ONE JSON line:
  build_device_ms    the build's kernels (HIP events, hry_bvh_stat): live flags, codes, four sort passes, tree, depth, leaves, box fit
  build_wall_ms      Codec.bvh as a caller sees it: the render build, the hierarchy, the render build freed
  primary_ms / primary_mrays     a 1024 x 1024 pinhole image of primary rays from outside the torus: the cast's kernel, and rays / time
  incoherent_ms / incoherent_mrays   as many random rays from a sphere about the scene towards points of its box, in no order
  primary_hits / incoherent_hits, primary_box_tests / incoherent_box_tests (per ray)
  checked / mismatches   a subset of the incoherent rays against a chunked float64 torch brute force of the contract's rule (the leaf
                     box's interval, then the hit; every triangle): the rays whose triangle, t or uv differ in any bit
  triangles / leaves / dead / distinct_codes / depth   the summary
Warm-up runs first, then medians over the repeats, with the smallest and largest run beside them ("_range").  No threshold is set
on any of these."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from harry_amd import codec as hc  # noqa: E402
from harry_amd import meshgen as mg  # noqa: E402


def pinhole(torch, side):
    """side x side primary rays from (0, -3, 1.8) towards the origin, 50 degrees across: (the eye [3], directions [side * side, 3])"""
    eye = torch.tensor([0.0, -3.0, 1.8], device="cuda")
    fwd = -eye / eye.norm()
    right = torch.linalg.cross(fwd, torch.tensor([0.0, 0.0, 1.0], device="cuda"))
    right = right / right.norm()
    up = torch.linalg.cross(right, fwd)
    s = torch.linspace(-0.4663, 0.4663, side, device="cuda")   # tan(25 degrees)
    d = fwd[None, None, :] + s[None, :, None] * right[None, None, :] - s[:, None, None] * up[None, None, :]
    return eye, d.reshape(-1, 3).contiguous()


def incoherent(torch, n, lo, hi, seed=1):
    g = torch.Generator(device="cuda").manual_seed(seed)
    mid, half = (lo + hi) / 2, (hi - lo) / 2
    v = torch.randn(n, 3, device="cuda", generator=g)
    o = mid + 2.5 * half.norm() * v / v.norm(dim=1, keepdim=True)
    aim = mid + 1.5 * half * (2 * torch.rand(n, 3, device="cuda", generator=g) - 1)
    return o.contiguous(), (aim - o).contiguous()


def brute_force(torch, buffers, o, d, chunk=8):
    """the contract's rule for every (ray, leaf) in float64, every operation a kernel of its own -> (tri int32, t, uv float32)"""
    f64 = torch.float64
    box, P, tri_of = buffers["leaf_box"].to(f64), buffers["leaf_positions"].to(f64).reshape(-1, 3, 3), buffers["leaf_tri"].to(torch.int64)
    lo, hi, inf = box[None, :, :3], box[None, :, 3:], float("inf")
    dot = lambda a, b: (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]
    cross = lambda a, b: torch.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                                      a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], dim=-1)
    out_tri, out_t, out_uv = [], [], []
    for at in range(0, len(o), chunk):
        O, D = o[at:at + chunk].to(f64)[:, None, :], d[at:at + chunk].to(f64)[:, None, :]
        inv = 1.0 / D
        a, c = (lo - O) * inv, (hi - O) * inv
        flat = D == 0
        outside = (flat & ((O < lo) | (O > hi))).any(dim=2)
        n = torch.where(flat, -inf, torch.minimum(a, c)).amax(dim=2)
        f = torch.where(flat, inf, torch.maximum(a, c)).amin(dim=2)
        near, far = torch.clamp(n - n.abs() * 2.0 ** -30, min=0.0), f + f.abs() * 2.0 ** -30
        e1, e2 = (P[:, 1] - P[:, 0])[None], (P[:, 2] - P[:, 0])[None]
        p = cross(D, e2)
        det = dot(e1, p)
        s = O - P[None, :, 0]
        q = cross(s, e1)
        u, v, tt = dot(s, p) / det, dot(D, q) / det, dot(e2, q) / det
        ok = ~outside & (near <= far) & torch.isfinite(det) & (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (near <= tt) & (tt <= far)
        tt = torch.where(ok, tt, inf)
        best = tt.amin(dim=1, keepdim=True)
        leaf = torch.where(ok & (tt == best), tri_of[None, :], 1 << 40).argmin(dim=1)
        hit = ok.any(dim=1)
        k = torch.arange(len(leaf), device=leaf.device)
        out_tri.append(torch.where(hit, tri_of[leaf], -1).to(torch.int32))
        out_t.append(torch.where(hit, tt[k, leaf], inf).to(torch.float32))
        out_uv.append(torch.where(hit[:, None], torch.stack([u[k, leaf], v[k, leaf]], dim=1), 0.0).to(torch.float32))
    return torch.cat(out_tri), torch.cat(out_t), torch.cat(out_uv)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--side", type=int, default=708, help="torus grid side; 708 -> 1 002 528 triangles (configs[1])")
    ap.add_argument("--image", type=int, default=1024, help="the image's side: image * image rays in either set")
    ap.add_argument("--check", type=int, default=4096, help="rays of the incoherent set that go through the brute force")
    args = ap.parse_args()
    import torch
    torch.cuda.init()   # torch holds the device before the codec starts
    cx = hc.Codec(0)
    try:
        g = mg.torus(args.side, args.side, seed=2, sigma=1e-4)
        m = hc.Mesh.from_arrays(g.verts, g.degrees, g.indices)
        cx.requant(m, [(1, -1, 14)])
        cfg1 = cx.write_hry(m, profile=hc.PROFILE_CHUNKED)
        dev, wall = [], []
        b = None
        for i in range(args.warmup + args.repeats):
            mesh = cx.read_hry(cfg1)
            if b is not None:
                b.close()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            b = cx.bvh(mesh)
            t1 = time.perf_counter()
            st = cx.bvh_stat()
            assert st["uploaded_bytes"] == 0
            if i >= args.warmup:
                dev.append(st["device_ms"])
                wall.append((t1 - t0) * 1e3)
        buffers = b.buffers()
        scene = buffers["scene_box"][0]
        eye, primary = pinhole(torch, args.image)
        o, d = incoherent(torch, args.image * args.image, scene[:3], scene[3:])
        res = {"ntris": int(g.ntri), "rays": args.image * args.image, "build_device_ms": statistics.median(dev), "build_device_ms_range": [min(dev), max(dev)],
               "build_wall_ms": statistics.median(wall), "build_wall_ms_range": [min(wall), max(wall)]}
        for name, (oo, dd) in (("primary", (eye, primary)), ("incoherent", (o, d))):
            ms = []
            for i in range(args.warmup + args.repeats):
                got = b.cast(oo, dd)
                if i >= args.warmup:
                    ms.append(b.device_ms)
            res.update({f"{name}_ms": statistics.median(ms), f"{name}_ms_range": [min(ms), max(ms)], f"{name}_mrays": len(dd) / statistics.median(ms) / 1e3,
                        f"{name}_hits": b.hits, f"{name}_box_tests": b.box_tests / len(dd)})
        n = min(args.check, len(d))
        if n:
            pick = torch.arange(n, device="cuda") * (len(d) // n)
            tri, t, uv = brute_force(torch, buffers, o[pick], d[pick])
            differ = (tri != got["tri"][pick]) | (t.view(torch.int32) != got["t"][pick].view(torch.int32)) | \
                     (uv.view(torch.int32) != got["uv"][pick].view(torch.int32)).any(dim=1)
            res.update({"checked": n, "checked_hits": int((tri >= 0).sum()), "mismatches": int(differ.sum())})
        res.update({k: st[k] for k in hc.Bvh.SUMMARY})
        print(json.dumps(res))
        b.close()
    finally:
        cx.close()


if __name__ == "__main__":
    main()
