"""Tangent frames of a render build (hry_tangents_build) on configs[1] with a parametric uv (1 002 528 triangles, x y z u v, -l1 -q14,
chunked container), through Codec.tangents, beside the plain torch way on the same tensors.  Prints ONE JSON line:
  device_ms_area / device_ms_angle   the tangents kernels' device_ms (HIP events, hry_tangents_stat), uv-area and corner-angle weights
  wall_ms_area / wall_ms_angle       Codec.tangents as a caller sees it: render build with normals, tangents build and the copies into
                                     torch tensors
  torch_ms                           the pass it replaces: float32 per-triangle terms, three index_add_ (float atomics) per sum,
                                     Gram-Schmidt against the normals and the handedness; torch.cuda events
Each Codec.tangents follows a fresh decode (the render build it starts from reads the decode's buffers in place); warm-up runs first,
then medians over the repeats, with the smallest and largest run beside them ("_range").  The last three keys say how far the torch
pass lies from the build on the framed vertices: rows off by more than 1e-3 in a tangent component, the median distance, and rows
with another handedness."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    args = ap.parse_args()
    import torch
    torch.cuda.init()   # torch holds the device before the codec starts
    cx = hc.Codec(0)
    try:
        nu = nv = 708
        g = mg.torus(nu, nv, seed=2, sigma=1e-4)
        iu, iv = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
        verts = np.zeros(g.nv, np.dtype([(k, "<f4") for k in ("x", "y", "z", "u", "v")]))
        for k in "xyz":
            verts[k] = g.verts[k]
        verts["u"], verts["v"] = (iv / nv).ravel(), (iu / nu).ravel()   # (one vertex per grid point: the wrap's cells stretch across the map)
        m = hc.Mesh.from_arrays(verts, g.degrees, g.indices)
        cx.requant(m, [(1, -1, 14)])
        cfg1 = cx.write_hry(m, profile=hc.PROFILE_CHUNKED)
        res, got = {}, None
        for key in ("area", "angle"):
            dev, wall = [], []
            for i in range(args.warmup + args.repeats):
                mesh = cx.read_hry(cfg1)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got = cx.tangents(mesh, normals="area", weights=key)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                assert cx.tangents_stat()["uploaded_bytes"] == 0 and cx.tangents_stat()["render_uploaded_bytes"] == 0
                if i >= args.warmup:
                    dev.append(cx.tangents_stat()["device_ms"])
                    wall.append((t1 - t0) * 1e3)
            res["device_ms_" + key], res["wall_ms_" + key] = statistics.median(dev), statistics.median(wall)
            res["device_ms_" + key + "_range"], res["wall_ms_" + key + "_range"] = [min(dev), max(dev)], [min(wall), max(wall)]
        st = cx.tangents_stat()
        res.update({k: st[k] for k in ("framed", "unframed", "mirrored", "mixed", "degenerate")})

        area = cx.tangents(cx.read_hry(cfg1), normals="area")
        r = cx.render(cx.read_hry(cfg1), normals="area")
        P, UV, N, idx = r["list1"][:, :3].contiguous(), r["list1"][:, 3:5].contiguous(), r["normals"], r["indices"].long()
        res["ntris"], res["nverts"] = int(idx.shape[0]), int(P.shape[0])

        def baseline():
            i0, i1, i2 = idx[:, 0], idx[:, 1], idx[:, 2]
            e1, e2 = P[i1] - P[i0], P[i2] - P[i0]
            d1, d2 = UV[i1] - UV[i0], UV[i2] - UV[i0]
            det = d1[:, 0] * d2[:, 1] - d2[:, 0] * d1[:, 1]
            s = torch.sign(det)[:, None]
            Tr = (e1 * d2[:, 1:2] - e2 * d1[:, 1:2]) * s
            Br = (e2 * d1[:, 0:1] - e1 * d2[:, 0:1]) * s
            S_T, S_B = torch.zeros_like(P), torch.zeros_like(P)
            for i in (i0, i1, i2):
                S_T.index_add_(0, i, Tr)
                S_B.index_add_(0, i, Br)
            R = S_T - N * (N * S_T).sum(dim=1, keepdim=True)
            t = R / R.norm(dim=1, keepdim=True)
            w = torch.where((torch.cross(N, t, dim=1) * S_B).sum(dim=1) < 0, -1.0, 1.0)
            return torch.cat([t, w[:, None]], dim=1)

        ms = []
        for i in range(args.warmup + args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = baseline()
            b.record()
            b.synchronize()
            if i >= args.warmup:
                ms.append(a.elapsed_time(b))
        res["torch_ms"], res["torch_ms_range"] = statistics.median(ms), [min(ms), max(ms)]
        # (float32 sums in the order the atomics completed in: where the map folds over -- the mixed vertices of the wrap -- the sums
        # nearly cancel and the two disagree at will; elsewhere they agree to float32's precision)
        framed = area["tangents"].abs().sum(dim=1) > 0
        off = (out[framed, :3] - area["tangents"][framed, :3]).abs().amax(dim=1)
        res["vertices_off_torch_by_1e-3"] = int((off > 1e-3).sum())
        res["median_difference_from_torch"] = float(off.median())
        res["handedness_differs_from_torch"] = int((out[framed, 3] != area["tangents"][framed, 3]).sum())
        print(json.dumps(res))
    finally:
        cx.close()


if __name__ == "__main__":
    main()
