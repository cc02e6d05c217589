"""Edges and adjacency of a render build (hry_edges_build) on configs[1] (1 002 528 triangles, -l1 -q14, chunked container), through
Codec.edges, beside the plain torch way on the same tensors.  Prints ONE JSON line:
  device_ms_topology / device_ms_geometry   the edges kernels' device_ms (HIP events, hry_edges_stat), without and with HRY_EDGES_GEOMETRY
  wall_ms_topology / wall_ms_geometry       Codec.edges as a caller sees it: render build, edges build and the copies into torch tensors
  torch_unique_ms / torch_geometry_ms       torch.unique(dim=0, return_inverse=True) over the 3 T sorted (min, max) index pairs; the same
                                            plus the gathers for length and cotangent (float32, index_add_); torch.cuda events
Each Codec.edges follows a fresh decode (the render build it starts from reads the decode's buffers in place); warm-up runs first,
then medians over the repeats, with the smallest and largest run beside them ("_range")."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from harry_amd import codec as hc  # noqa: E402
from harry_amd import meshgen as mg  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    args = ap.parse_args()
    import torch
    torch.cuda.init()   # torch holds the device before the codec starts
    cx = hc.Codec(0)
    try:
        m = hc.Mesh.from_ply(mg.torus(708, 708, seed=2, sigma=1e-4).to_ply())
        cx.requant(m, [(1, -1, 14)])
        cfg1 = cx.write_hry(m, profile=hc.PROFILE_CHUNKED)
        res, got = {}, None
        for key, geometry in (("topology", False), ("geometry", True)):
            dev, wall = [], []
            for i in range(args.warmup + args.repeats):
                mesh = cx.read_hry(cfg1)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got = cx.edges(mesh, geometry=geometry)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                assert cx.edges_stat()["uploaded_bytes"] == 0
                if i >= args.warmup:
                    dev.append(cx.edges_stat()["device_ms"])
                    wall.append((t1 - t0) * 1e3)
            res["device_ms_" + key], res["wall_ms_" + key] = statistics.median(dev), statistics.median(wall)
            res["device_ms_" + key + "_range"] = [min(dev), max(dev)]
        st = cx.edges_stat()
        res.update({k: st[k] for k in ("edges", "boundary", "manifold", "nonmanifold")})

        r = cx.render(cx.read_hry(cfg1))
        P, idx = r["list1"][:, :3].contiguous(), r["indices"].long()
        res["ntris"] = int(idx.shape[0])

        def baseline(geometry):
            a, b = idx.reshape(-1), idx[:, [1, 2, 0]].reshape(-1)
            pairs = torch.stack([torch.minimum(a, b), torch.maximum(a, b)], dim=1)
            uniq, inv = torch.unique(pairs, dim=0, return_inverse=True)
            if not geometry:
                return uniq, inv
            length = (P[uniq[:, 1]] - P[uniq[:, 0]]).norm(dim=1)
            o = idx[:, [2, 0, 1]].reshape(-1)
            u, v = P[a] - P[o], P[b] - P[o]
            c = (u * v).sum(dim=1) / torch.cross(u, v, dim=1).norm(dim=1)
            cot = 0.5 * torch.zeros(len(uniq), device=P.device).index_add_(0, inv, c)
            return uniq, inv, length, cot

        for key, geometry in (("torch_unique_ms", False), ("torch_geometry_ms", True)):
            ms = []
            for i in range(args.warmup + args.repeats):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                out = baseline(geometry)
                b.record()
                b.synchronize()
                if i >= args.warmup:
                    ms.append(a.elapsed_time(b))
            res[key] = statistics.median(ms)
            res[key + "_range"] = [min(ms), max(ms)]
        assert len(out[0]) == len(got["edges"])   # the same edges, in torch's sorted order
        res["largest_cot_difference"] = float((torch.sort(out[3])[0] - torch.sort(got["edge_cot"])[0]).abs().max())
        print(json.dumps(res))
    finally:
        cx.close()


if __name__ == "__main__":
    main()
