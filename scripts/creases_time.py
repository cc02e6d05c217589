"""Hard edges and split normals of a render build (hry_creases_build) on configs[1] (1 002 528 triangles, -l1 -q14, chunked
container), resident after a decode, through Codec.creases.  Prints ONE JSON line; per limit (cos_limit -1: everything smooth, cos 30
degrees, 2: flat shading) under the keys "smooth", "deg30" and "flat":
  device_ms          the creases kernels' device_ms (HIP events, hry_creases_stat)
  edges_device_ms    the edges build with geometry before it, on the same run (hry_edges_stat)
  wall_ms            Codec.creases as a caller sees it: render build, edges build, creases build, the copies into torch tensors and the
                     gather of the positions
  vertices / groups / smooth / sharp / split / other   hry_creases_summary
and once, "render_normals_device_ms": the render build with vertex normals on the same decode (hry_render_stat), the smooth normals
the creases build takes the place of.  Each Codec.creases follows a fresh decode (the render build it starts from reads the decode's
buffers in place); warm-up runs first, then medians over the repeats, with the smallest and largest run beside them ("_range").  No
threshold is set on any of these."""
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
        res = {"ntris": int(g.ntri)}
        for key, limit in (("smooth", -1.0), ("deg30", math.cos(math.radians(30.0))), ("flat", 2.0)):
            dev, edges, wall = [], [], []
            for i in range(args.warmup + args.repeats):
                mesh = cx.read_hry(cfg1)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                cx.creases(mesh, cos_limit=limit)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                st = cx.creases_stat()
                assert st["uploaded_bytes"] == 0 and st["render_uploaded_bytes"] == 0
                if i >= args.warmup:
                    dev.append(st["device_ms"])
                    edges.append(st["edges_device_ms"])
                    wall.append((t1 - t0) * 1e3)
            res[key] = {"cos_limit": limit, "device_ms": statistics.median(dev), "device_ms_range": [min(dev), max(dev)],
                        "edges_device_ms": statistics.median(edges), "edges_device_ms_range": [min(edges), max(edges)],
                        "wall_ms": statistics.median(wall), "wall_ms_range": [min(wall), max(wall)],
                        **{k: st[k] for k in hc.Codec.CREASES_SUMMARY}}
        ms = []
        for i in range(args.warmup + args.repeats):
            cx.render(cx.read_hry(cfg1), normals="area")
            if i >= args.warmup:
                ms.append(cx.render_stat()["device_ms"])
        res["render_normals_device_ms"], res["render_normals_device_ms_range"] = statistics.median(ms), [min(ms), max(ms)]
        print(json.dumps(res))
    finally:
        cx.close()


if __name__ == "__main__":
    main()
