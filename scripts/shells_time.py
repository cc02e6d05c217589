"""Shells of a render build (hry_shells_build) through Codec.shells, on two meshes resident after a decode, beside two other ways to
the same labels from the same edges data.  Meshes: configs[1] (1 002 528 triangles in ONE shell, -l1 -q14, chunked container: the worst
case for the union-find's root and for the ordered sums) and multi_component(64, 88, 89) (64 shells).  Prints ONE JSON line, per mesh:
  device_ms_topology / device_ms_geometry   the shells kernels' device_ms (HIP events, hry_shells_stat), without and with HRY_SHELLS_GEOMETRY
  wall_ms_topology / wall_ms_geometry       Codec.shells as a caller sees it: render, edges and shells builds and the copies into torch tensors
  torch_propagate_ms                        a torch min-label propagation loop on the device over Codec.edges' tri_edges, until nothing
                                            changes: every edge takes the least label of its sides (scatter_reduce amin), every triangle
                                            the least of its edges; the loop's passes are counted in torch_propagate_passes
  torch_jump_ms                             the same loop with a pointer jump (label = label[label]) after every pass
  scipy_ms                                  where scipy imports: scipy.sparse.csgraph.connected_components on the host over the
                                            (side, first side of its edge) pairs, including the copy down of tri_edges / edge_offsets / edge_sides
Each Codec.shells follows a fresh decode; warm-up runs first, then medians over the repeats, with the smallest and largest run beside
them ("_range").  The baselines give labels only: no counts, loops or measures, and their numbering is not by lowest triangle."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from harry_amd import codec as hc  # noqa: E402
from harry_amd import meshgen as mg  # noqa: E402


def measure(cx, torch, blob, args):
    res = {}
    got = None
    for key, geometry in (("topology", False), ("geometry", True)):
        dev, wall = [], []
        for i in range(args.warmup + args.repeats):
            mesh = cx.read_hry(blob)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = cx.shells(mesh, geometry=geometry)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            assert cx.shells_stat()["uploaded_bytes"] == 0
            if i >= args.warmup:
                dev.append(cx.shells_stat()["device_ms"])
                wall.append((t1 - t0) * 1e3)
        res["device_ms_" + key], res["wall_ms_" + key] = statistics.median(dev), statistics.median(wall)
        res["device_ms_" + key + "_range"], res["wall_ms_" + key + "_range"] = [min(dev), max(dev)], [min(wall), max(wall)]
    st = cx.shells_stat()
    res.update({k: st[k] for k in ("shells", "closed", "nonmanifold", "misoriented", "loops", "largest")})

    e = cx.edges(cx.read_hry(blob))
    te = e["tri_edges"].long().reshape(-1)
    T, E = te.numel() // 3, int(e["edges"].shape[0])
    res["ntris"] = T

    def propagate(jump):
        label = torch.arange(T, device=te.device)
        passes = 0
        while True:
            per_edge = torch.full((E,), T, device=te.device).scatter_reduce_(0, te, label.repeat_interleave(3), "amin")
            new = torch.minimum(label, per_edge[te].reshape(T, 3).amin(dim=1))
            if jump:
                new = new[new]
            passes += 1
            if torch.equal(new, label):
                return label, passes
            label = new

    for key, jump in (("torch_propagate", False), ("torch_jump", True)):
        ms = []
        for i in range(args.warmup + args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            label, passes = propagate(jump)
            b.record()
            b.synchronize()
            if i >= args.warmup:
                ms.append(a.elapsed_time(b))
        res[key + "_ms"], res[key + "_ms_range"], res[key + "_passes"] = statistics.median(ms), [min(ms), max(ms)], passes
        assert int(torch.unique(label).numel()) == st["shells"]
        first = torch.zeros(st["shells"], dtype=torch.long, device=te.device).scatter_(0, got["tri_shell"].long(), label)
        assert torch.equal(first[got["tri_shell"].long()], label) and torch.equal(first, got["shell_first"].long())   # the same partition, the same roots

    try:
        import numpy as np
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
    except ImportError:
        return res
    ms = []
    for i in range(args.warmup + args.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h_te, h_off, h_sides = e["tri_edges"].cpu().numpy().reshape(-1), e["edge_offsets"].cpu().numpy(), e["edge_sides"].cpu().numpy()
        first_side = h_sides[h_off[:-1]][h_te]
        g = coo_matrix((np.ones(3 * T, np.int8), (np.arange(3 * T) // 3, first_side // 3)), shape=(T, T))
        n, lab = connected_components(g, directed=False)
        t1 = time.perf_counter()
        if i >= args.warmup:
            ms.append((t1 - t0) * 1e3)
    assert n == st["shells"]
    res["scipy_ms"], res["scipy_ms_range"] = statistics.median(ms), [min(ms), max(ms)]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    args = ap.parse_args()
    import torch
    torch.cuda.init()   # torch holds the device before the codec starts
    cx = hc.Codec(0)
    try:
        out = {}
        for name, make in (("configs1", lambda: mg.torus(708, 708, seed=2, sigma=1e-4)), ("multi64", lambda: mg.multi_component(64, 88, 89))):
            m = hc.Mesh.from_ply(make().to_ply())
            cx.requant(m, [(1, -1, 14)])
            out[name] = measure(cx, torch, cx.write_hry(m, profile=hc.PROFILE_CHUNKED), args)
        print(json.dumps(out))
    finally:
        cx.close()


if __name__ == "__main__":
    main()
