"""The numpy restatement of hry_intersections_build (include/harry_amd.h): the pairs of a hierarchy's triangles that pass through each
other, by a brute force over all pairs of leaves -- the boxes on the floats, proper triangles, corners shared by position, the admitted
edges of one against the other with the arithmetic of the cast's hit.  Nothing here walks a tree but `walk`, the reference stack
walk the CPU tests compare with the brute force and count box tests with.  Every floating-point operation is a numpy double
operation of its own, in the order the contract writes them -- (a*b + c*d) + e*f --, so the device must agree bit for bit.  `bvh` is
a hierarchy of tests/bvh_ref.py (or the buffers of a Bvh with "summary")."""
import numpy as np

from tests import bvh_ref as br

BUFFERS = ("pairs", "pair_shared", "tri_pairs")
SUMMARY = ("triangles", "candidates", "tested", "pairs", "triangles_hit")   # and the box tests, which depend on the walk


def corners(bvh):
    """the leaves' corners as doubles [L, 3, 3] (corner, axis)"""
    return bvh["leaf_positions"].astype(np.float64).reshape(-1, 3, 3)


def proper(P):
    """n = (P1 - P0) x (P2 - P0), n . n > 0"""
    with np.errstate(all="ignore"):
        n = br.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
        return br.dot(n, n) > 0


def meets(a, b, tri):
    """the segments (a, b) [n, 3] against the triangles tri [n, 3, 3]: the cast's hit with o = a, d = b - a and 0 <= tt <= 1"""
    with np.errstate(all="ignore"):
        d = b - a
        e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
        p = br.cross(d, e2)
        det = br.dot(e1, p)
        s = a - tri[:, 0]
        q = br.cross(s, e1)
        u, v, tt = br.dot(s, p) / det, br.dot(d, q) / det, br.dot(e2, q) / det
        return np.isfinite(det) & (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (0 <= tt) & (tt <= 1)


def boxes_meet(a, b):
    """closed, on the floats: lo_a <= hi_b and lo_b <= hi_a on the three axes (broadcasting)"""
    return ((a[..., :3] <= b[..., 3:]) & (b[..., :3] <= a[..., 3:])).all(axis=-1)


def decide(bvh, i, j):
    """the candidates: leaves i, j (arrays) with leaf_tri[i] < leaf_tri[j] whose boxes overlap -> the result.  Clauses 2 and 3"""
    T = int(bvh["summary"][0])
    P = corners(bvh)
    A, B = P[i], P[j]
    same = (A[:, :, None, :] == B[:, None, :, :]).all(axis=3)   # [n, corner of A, corner of B]: -0 equals +0
    share = same.any(axis=2).sum(axis=1)
    ok = proper(A) & proper(B)
    reach = ok & (share <= 1)
    ka, kb = same.any(axis=2).argmax(axis=1), same.any(axis=1).argmax(axis=1)   # the shared corner on either side, where share == 1
    hit = np.zeros(len(i), bool)
    rows = np.arange(len(i))
    for k in range(3):
        # edge k is (P_k, P_(k + 1) % 3); with one shared corner only the edge opposite it, which begins at the corner behind it
        admit_a = (share == 0) | ((share == 1) & ((ka + 1) % 3 == k))
        admit_b = (share == 0) | ((share == 1) & ((kb + 1) % 3 == k))
        hit |= admit_a & meets(A[rows, k], A[rows, (k + 1) % 3], B)
        hit |= admit_b & meets(B[rows, k], B[rows, (k + 1) % 3], A)
    hit &= reach
    t, s = bvh["leaf_tri"][i][hit].astype(np.uint32), bvh["leaf_tri"][j][hit].astype(np.uint32)
    order = np.lexsort((s, t))
    pairs = np.stack([t[order], s[order]], axis=1).reshape(-1, 2).astype(np.uint32)
    tri_pairs = (np.bincount(t.astype(np.int64), minlength=T) + np.bincount(s.astype(np.int64), minlength=T)).astype(np.uint32)[:T]
    return {"pairs": pairs, "pair_shared": share[hit][order].astype(np.uint32), "tri_pairs": tri_pairs,
            "summary": (T, len(i), int(reach.sum()), len(pairs), int((tri_pairs > 0).sum()))}


def intersections(bvh, chunk=512):
    """every leaf against every leaf -> "pairs" u32 [P, 2], "pair_shared" u32 [P], "tri_pairs" u32 [T], "summary" (T, C, N, P, H)"""
    box, tri = bvh["leaf_box"], bvh["leaf_tri"].astype(np.int64)
    L = len(tri)
    ii, jj = [], []
    for at in range(0, L, chunk):
        m = boxes_meet(box[at:at + chunk, None, :], box[None, :, :]) & (tri[at:at + chunk, None] < tri[None, :])
        a, b = np.nonzero(m)
        ii.append(a + at)
        jj.append(b)
    i = np.concatenate(ii) if ii else np.zeros(0, np.int64)
    j = np.concatenate(jj) if jj else np.zeros(0, np.int64)
    return decide(bvh, i.astype(np.int64), j.astype(np.int64))


def walk(bvh):
    """every leaf down the tree with a stack, in plain Python floats: a node's two children's boxes against the leaf's, leaf children
    answered at once (on the side of the lower triangle number), internal ones pushed -> (the result, box tests made)"""
    L = len(bvh["leaf_tri"])
    leaf_box, node_box = bvh["leaf_box"].astype(np.float64).tolist(), bvh["node_box"].astype(np.float64).tolist()   # (floats widen exactly)
    children, tri = bvh["node_children"].tolist(), bvh["leaf_tri"].tolist()
    tests, deepest = 0, 0
    ii, jj = [], []

    def meet(a, b):
        return a[0] <= b[3] and b[0] <= a[3] and a[1] <= b[4] and b[1] <= a[4] and a[2] <= b[5] and b[2] <= a[5]

    for i in range(L if L > 1 else 0):
        mine, t = leaf_box[i], tri[i]
        stack = [0]
        while stack:
            deepest = max(deepest, len(stack))
            node = stack.pop()
            for c in children[node]:
                n = c & ~br.LEAF
                tests += 1
                if not meet(mine, leaf_box[n] if c & br.LEAF else node_box[n]):
                    continue
                if not c & br.LEAF:
                    stack.append(n)
                elif t < tri[n]:
                    ii.append(i)
                    jj.append(n)
    assert deepest <= 64
    return decide(bvh, np.array(ii, np.int64), np.array(jj, np.int64)), tests


def of_triangles(triangles):
    """the hierarchy over triangles given as nine floats each, on vertices of their own: [[x0, y0, z0, x1, ...], ...]"""
    pos = np.asarray(triangles, np.float32).reshape(-1, 3)
    return br.build(np.arange(len(pos), dtype=np.uint32).reshape(-1, 3), pos)
