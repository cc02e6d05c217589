"""Designed symbol planes (tests/planes_ref.py) through the chunked container's coders on the GPU, every check exact against the CPU
oracle: k_plane_hist, k_chunk_encode or k_chunk_model + k_chunk_ranges on the way in, k_chunk_decode or k_chunk_decode_lanes
<16 / 32-bit counts> on the way out.  The decoder form is this process' (HRY_DECODE_LANES and HRY_DECODE_COUNTS32 are read once);
the encoder form changes between encodes (HRY_ENCODE_SPLIT_MIN_STREAMS is read per call).  The stages "enc_plan" and "dec_plan"
say which kernels ran, and are checked: a case means nothing if the kernel it names stayed idle.  One line per case, then
"all equal"; the first mismatch ends the run, named by case, plane and first differing symbol.
    HRY_DECODE_LANES=1 python tests/tools/plane_cases.py [case ...]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from harry_amd import codec as hc
from oracle import oracle_py as op   # checker only
from tests import planes_ref as pr

lanes_env, wide_env = os.environ.get("HRY_DECODE_LANES"), os.environ.get("HRY_DECODE_COUNTS32")
if lanes_env not in ("0", "1"):
    sys.exit("set HRY_DECODE_LANES to 0 (a wavefront per stream) or 1 (a lane per stream)")
FORM = "waves" if lanes_env == "0" else "lanes32" if wide_env else "lanes"
only = sys.argv[1:]
cx = hc.Codec(0)


class Mismatch(Exception):
    pass


def fail(case, what):
    raise Mismatch(f"{case}: {what}")


def planes_equal(case, what, got, want, names=None):
    """got, want: (planes, symbols)"""
    if got.shape != want.shape:
        fail(case, f"{what}: shape {got.shape}, expected {want.shape}")
    bad = np.argwhere(got != want)
    if len(bad):
        p, i = (int(x) for x in bad[0])
        fail(case, f"{what}: plane {names[p] if names else p}, first differing symbol {i}: {int(got[p, i])}, expected {int(want[p, i])} ({len(bad)} differ)")


def check(case, cond, what):
    if not cond:
        fail(case, what)


def run_case(case, mesh_name, chunk, compat_too, built):
    if mesh_name not in built:   # the mesh and the oracle's side of it: once, shared by the cases and both encoder forms
        mesh, seqs = pr.case_mesh(mesh_name)
        ply = mesh.to_ply()
        o = op.Mesh.from_ply(ply)
        compat = o.clone().encode().data
        built.clear()            # (one mesh at a time)
        built[mesh_name] = (ply, seqs, o, compat, op.Mesh.from_hry(compat))
    ply, seqs, o, compat, ref = built[mesh_name]
    want_f = np.stack(seqs)                       # (planes, faces): the face planes as designed
    check(case, np.array_equal(ref.list_data(0), want_f.T), "the reference-format decode does not return the designed planes")
    lines = []
    for split in ("0", "1"):
        os.environ["HRY_ENCODE_SPLIT_MIN_STREAMS"] = split
        tag = f"{case} [{FORM}, encoder {'two kernels' if split == '1' else 'one kernel'} asked]"
        a = hc.Mesh.from_ply(ply)
        got = cx.write_hry(a.clone(), profile=hc.PROFILE_CHUNKED, chunk_syms=chunk, keep_stages=True)
        fplanes, vplanes, enc_plan = cx.stage("fplanes"), cx.stage("vplanes"), cx.stage("enc_plan", np.uint32)
        planes_equal(tag, "fplanes of the encode", fplanes.reshape(len(seqs), -1), want_f)
        info = hc.container_info(got)
        want = o.clone().encode_chunked(info["chunk_syms"])
        check(tag, chunk == 0 or info["chunk_syms"] == chunk, "chunk_syms of the container")
        if got != want.data:
            g, w = np.frombuffer(got, np.uint8), np.frombuffer(want.data, np.uint8)
            n = min(len(g), len(w))
            d = np.flatnonzero(g[:n] != w[:n])
            fail(tag, f"container differs from the oracle's: {len(g)} bytes, expected {len(w)}, first differing byte {int(d[0]) if len(d) else n} (header {info['header_bytes']})")
        CH, CHC, nsym, tables = pr.directory(got, info["header_bytes"])
        t0 = [pr.initial_total(k, t) for k, t in enumerate(tables)]
        cuts = [pr.stream_lengths(k, int(n), CH, CHC) for k, n in enumerate(nsym)]
        top = pr.largest_total(got, info["header_bytes"])

        # ---- the encoder's plan
        ns, two, enc_top = (int(x) for x in enc_plan)
        check(tag, ns == sum(len(c) for c in cuts), f"enc_plan: {ns} streams, the directory cuts {sum(len(c) for c in cuts)}")
        check(tag, two == (1 if split == "1" and top <= 65535 else 0), f"enc_plan: two kernels = {two} with HRY_ENCODE_SPLIT_MIN_STREAMS={split} and a largest total of {top}")
        check(tag, enc_top == top, f"enc_plan: largest total {enc_top}, the directory says {top}")

        # ---- decode, plane by plane
        dec = cx.read_hry(got, keep_stages=True)
        syms, dn, dec_plan = cx.stage("dec_syms"), cx.stage("dec_nsym", np.uint32), cx.stage("dec_plan", np.uint32).reshape(-1, 3)
        check(tag, np.array_equal(dn, nsym), "dec_nsym is not the directory's")
        n_conn = int(nsym[:pr.N_CONN_PLANES].sum())
        tail = syms[n_conn:]
        check(tag, len(tail) == len(vplanes) + len(fplanes), "dec_syms: length")
        nv_planes = len(nsym) - pr.N_CONN_PLANES - len(seqs)
        planes_equal(tag, "decoded vertex planes", tail[:len(vplanes)].reshape(nv_planes, -1), vplanes.reshape(nv_planes, -1), [pr.N_CONN_PLANES + k for k in range(nv_planes)])
        planes_equal(tag, "decoded face planes", tail[len(vplanes):].reshape(len(seqs), -1), want_f, [pr.N_CONN_PLANES + nv_planes + k for k in range(len(seqs))])
        at12 = int(nsym[:12].sum())
        planes_equal(tag, "decoded numtri high bytes", syms[None, at12:at12 + int(nsym[12])], np.zeros((1, int(nsym[12])), np.uint8), [12])
        check(tag, (dec.nv, dec.nf, dec.ne) == (ref.nv, ref.nf, ref.ne), "decoded sizes")
        check(tag, np.array_equal(dec.org(), ref.org()), "decoded connectivity differs from the reference-format decode")
        check(tag, np.array_equal(dec.list_data(1), ref.list_data(1)), "decoded vertex list differs from the reference-format decode")
        planes_equal(tag, "decoded face list", np.ascontiguousarray(dec.list_data(0).T), want_f)

        # ---- the decoder's plan: row 0 the connectivity launch, the others the attribute groups'
        for_lanes = [sum(len(cuts[k]) for k in ks if t0[k] is not None and t0[k] > 128) for ks in (range(pr.N_CONN_PLANES), range(pr.N_CONN_PLANES, len(nsym)))]
        streams = [sum(len(cuts[k]) for k in ks) for ks in (range(pr.N_CONN_PLANES), range(pr.N_CONN_PLANES, len(nsym)))]
        check(tag, for_lanes[1] == streams[1], "an attribute plane whose streams no lane can decode")
        tops = [max([t0[k] + max(cuts[k]) for k in ks if t0[k] is not None and t0[k] > 128 and cuts[k]], default=0) for ks in (range(pr.N_CONN_PLANES), range(pr.N_CONN_PLANES, len(nsym)))]
        check(tag, tops[1] <= 65535, "attribute streams past the 16-bit limit: not what this case is for")
        check(tag, len(dec_plan) >= 2 and int(dec_plan[0, 0]) == streams[0] and int(dec_plan[1:, 0].sum()) == streams[1], f"dec_plan: streams {dec_plan[:, 0].tolist()}, expected {streams}")
        lanes = FORM != "waves"
        got_lanes = [int(dec_plan[0, 1]), int(dec_plan[1:, 1].sum())]
        check(tag, got_lanes == ([for_lanes[0], for_lanes[1]] if lanes else [0, 0]), f"dec_plan: {got_lanes} streams to the lanes, expected {for_lanes if lanes else [0, 0]}")
        c16 = 1 if FORM == "lanes" and for_lanes[0] and tops[0] <= 65535 else 0
        check(tag, int(dec_plan[0, 2]) == c16, f"dec_plan: counts16 = {int(dec_plan[0, 2])} for connectivity totals up to {tops[0]}")
        for row in dec_plan[1:]:
            check(tag, int(row[2]) == (1 if FORM == "lanes" and row[1] else 0), f"dec_plan: attribute row {row.tolist()}")

        # ---- the reference-format profile: its model kernels count by ballot the same way
        if compat_too:
            check(tag, cx.write_hry(a.clone(), profile=hc.PROFILE_COMPAT) == compat, "reference-format stream differs from the oracle's")
            d2 = cx.read_hry(compat)
            check(tag, np.array_equal(d2.org(), ref.org()) and np.array_equal(d2.list_data(1), ref.list_data(1)), "decode of the reference-format stream")
            planes_equal(tag, "face list decoded from the reference-format stream", np.ascontiguousarray(d2.list_data(0).T), want_f)
        lines.append(f"enc {'two' if two else 'one'} top {enc_top} dec conn {dec_plan[0].tolist()} attr {[int(x) for x in dec_plan[1:].sum(axis=0)[:2]]}")
    return "; ".join(lines)


t_start = time.time()
built = {}
try:
    for case, mesh_name, chunk, compat_too in pr.CASES:
        if only and case not in only:
            continue
        t = time.time()
        line = run_case(case, mesh_name, chunk, compat_too, built)
        print(f"{case:16s} {FORM:8s} {line}  ({time.time() - t:.1f} s)", flush=True)
except Mismatch as e:
    print("MISMATCH", e, flush=True)
    sys.exit(1)
finally:
    os.environ.pop("HRY_ENCODE_SPLIT_MIN_STREAMS", None)
cx.close()
print(f"total {time.time() - t_start:.1f} s")
print("all equal")
