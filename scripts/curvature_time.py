"""Vertex areas and curvatures of a render build (hry_curvature_build) on configs[1] (1 002 528 triangles, -l1 -q14, chunked
container), resident after a decode, through Codec.curvature.  Prints ONE JSON line:
  device_ms          the curvature kernels' device_ms (HIP events, hry_curvature_stat)
  edges_device_ms    the edges build before it, on the same run (hry_edges_stat)
  wall_ms            Codec.curvature as a caller sees it: render build, edges build, curvature build and the copies into torch tensors
  torch_ms           what a caller had to write before: the same six quantities (class aside) in float32 torch on the render build's
                     tensors -- the corners' cotangents, angles and mixed-area shares per triangle, four index_add_ scatters (float
                     atomics: neither the order nor the bits are fixed) and the divisions -- timed by events around the pass
  vertices / interior / boundary / irregular / isolated / degenerate, area / defect / mean_integral   the summary and the totals
Each Codec.curvature follows a fresh decode (the render build it starts from reads the decode's buffers in place); warm-up runs
first, then medians over the repeats, with the smallest and largest run beside them ("_range").  No threshold is set on any of
these."""
import argparse
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from harry_amd import codec as hc  # noqa: E402
from harry_amd import meshgen as mg  # noqa: E402


def torch_curvature(torch, pos, idx, nv):
    """area, defect (interior tau everywhere: the baseline has no edges build), gaussian, mean_normal, mean -- float32, index_add_"""
    I = idx.long()
    p = [pos[I[:, k]] for k in range(3)]
    N = torch.linalg.cross(p[1] - p[0], p[2] - p[0])
    area_t = 0.5 * N.norm(dim=1)
    a = [p[(k + 1) % 3] - p[k] for k in range(3)]
    b = [p[(k + 2) % 3] - p[k] for k in range(3)]
    d = [(a[k] * b[k]).sum(dim=1) for k in range(3)]
    x = [torch.linalg.cross(a[k], b[k]).norm(dim=1) for k in range(3)]
    c = [torch.nan_to_num(d[k] / x[k], nan=0.0, posinf=0.0, neginf=0.0) for k in range(3)]
    obtuse = (d[0] < 0) | (d[1] < 0) | (d[2] < 0)
    theta = torch.zeros(nv, device=pos.device)
    A = torch.zeros(nv, device=pos.device)
    L = torch.zeros(nv, 3, device=pos.device)
    S = torch.zeros(nv, 3, device=pos.device)
    for k in range(3):
        cn, cp = c[(k + 1) % 3], c[(k + 2) % 3]
        share = torch.where(obtuse, torch.where(d[k] < 0, 0.5 * area_t, 0.25 * area_t),
                            0.125 * ((a[k] * a[k]).sum(dim=1) * cp + (b[k] * b[k]).sum(dim=1) * cn))
        theta.index_add_(0, I[:, k], torch.atan2(x[k], d[k]))
        A.index_add_(0, I[:, k], share)
        L.index_add_(0, I[:, k], -(cp[:, None] * a[k] + cn[:, None] * b[k]))
        S.index_add_(0, I[:, k], N)
    defect = 2 * math.pi - theta
    four = 4 * A
    return A, defect, defect / A, L / four[:, None], (L * S).sum(dim=1) / (S.norm(dim=1) * four)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--side", type=int, default=708, help="torus grid side; 708 -> 1 002 528 triangles (configs[1])")
    args = ap.parse_args()
    import torch
    torch.cuda.init()   # torch holds the device before the codec starts
    cx = hc.Codec(0)
    try:
        g = mg.torus(args.side, args.side, seed=2, sigma=1e-4)
        m = hc.Mesh.from_arrays(g.verts, g.degrees, g.indices)
        cx.requant(m, [(1, -1, 14)])
        cfg1 = cx.write_hry(m, profile=hc.PROFILE_CHUNKED)
        dev, edges, wall = [], [], []
        for i in range(args.warmup + args.repeats):
            mesh = cx.read_hry(cfg1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            cx.curvature(mesh)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            st = cx.curvature_stat()
            assert st["uploaded_bytes"] == 0
            if i >= args.warmup:
                dev.append(st["device_ms"])
                edges.append(st["edges_device_ms"])
                wall.append((t1 - t0) * 1e3)
        rt = cx.render(cx.read_hry(cfg1))
        pos, idx = rt["list1"][:, :3].contiguous(), rt["indices"]
        base = []
        for i in range(args.warmup + args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            torch_curvature(torch, pos, idx, len(pos))
            e1.record()
            torch.cuda.synchronize()
            if i >= args.warmup:
                base.append(e0.elapsed_time(e1))
        res = {"ntris": int(g.ntri), "device_ms": statistics.median(dev), "device_ms_range": [min(dev), max(dev)],
               "edges_device_ms": statistics.median(edges), "edges_device_ms_range": [min(edges), max(edges)],
               "wall_ms": statistics.median(wall), "wall_ms_range": [min(wall), max(wall)],
               "torch_ms": statistics.median(base), "torch_ms_range": [min(base), max(base)],
               **{k: st[k] for k in hc.Codec.CURVATURE_SUMMARY + hc.Codec.CURVATURE_TOTALS}}
        print(json.dumps(res))
    finally:
        cx.close()


if __name__ == "__main__":
    main()
