"""The numpy restatement of hry_bvh_build and hry_bvh_cast (include/harry_amd.h): the hierarchy by its definition -- codes,
np.lexsort, the radix tree by the rule of its split, boxes -- and the cast as a brute force of every ray against every leaf (the
interval of the leaf's box, then the hit).  Nothing here walks a tree to answer a ray but `walk`, the reference stack walk the CPU
tests compare with the brute force and count box tests with.  Every floating-point operation is a numpy double operation of its own,
in the order the contract writes them, so the device must agree bit for bit."""
import numpy as np

NO_ELEMENT = 0xFFFFFFFF
LEAF = 0x80000000
BUFFERS = ("leaf_tri", "leaf_code", "leaf_box", "leaf_positions", "node_children", "node_box", "scene_box")
SUMMARY = ("triangles", "leaves", "dead", "distinct_codes", "depth")
WIDEN = 2.0 ** -30


# ---- floats in their order with -0 below +0
def ordered(f):
    u = np.ascontiguousarray(f, np.float32).view(np.uint32)
    return np.where(u & 0x80000000, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def unordered(w):
    w = np.asarray(w, np.uint32)
    return np.where(w & 0x80000000, w ^ np.uint32(0x80000000), ~w).astype(np.uint32).view(np.float32)


def least(f, axis):
    return unordered(ordered(f).min(axis=axis))


def greatest(f, axis):
    return unordered(ordered(f).max(axis=axis))


# ---- the hierarchy
def spread3(x):
    x = x.astype(np.uint32)
    x = (x | (x << 16)) & 0x030000FF
    x = (x | (x << 8)) & 0x0300F00F
    x = (x | (x << 4)) & 0x030C30C3
    return (x | (x << 2)) & 0x09249249


def codes_of(tri_pos, lo, hi):
    """tri_pos f32 [n, 3, 3] (corner, axis) of live triangles; lo, hi f32 [3]"""
    p = tri_pos.astype(np.float64)
    c = ((p[:, 0] + p[:, 1]) + p[:, 2]) / 3.0
    lo64, hi64 = lo.astype(np.float64), hi.astype(np.float64)
    with np.errstate(all="ignore"):
        x = ((c - lo64) / (hi64 - lo64)) * 1024.0
    cell = np.where(hi == lo, 0.0, np.clip(np.trunc(np.where(hi == lo, 0.0, x)), 0.0, 1023.0)).astype(np.uint32)
    return (spread3(cell[:, 0]) << 2) | (spread3(cell[:, 1]) << 1) | spread3(cell[:, 2])


def tree_of(codes):
    """(children u32 [L - 1, 2], ranges i64 [L - 1, 2]) of the radix tree of the keys code_i * 2^32 + i, by the definition: a node
    that covers [a, b] splits behind the largest j in [a, b) whose key shares more leading bits with key_a than key_a with key_b"""
    L = len(codes)
    keys = (codes.astype(np.uint64) << np.uint64(32)) | np.arange(L, dtype=np.uint64)
    children = np.zeros((max(L - 1, 0), 2), np.uint32)
    ranges = np.zeros((max(L - 1, 0), 2), np.int64)
    todo = [(0, 0, L - 1)] if L >= 2 else []
    while todo:
        node, a, b = todo.pop()
        ranges[node] = (a, b)
        common = 64 - int(keys[a] ^ keys[b]).bit_length()
        x = keys[a:b] ^ keys[a]   # more than `common` leading bits shared: x < 2^(63 - common)
        gamma = a + int(np.flatnonzero(x < np.uint64(1 << (63 - common)))[-1])
        if a == gamma:
            children[node, 0] = gamma | LEAF
        else:
            children[node, 0] = gamma
            todo.append((gamma, a, gamma))
        if gamma + 1 == b:
            children[node, 1] = (gamma + 1) | LEAF
        else:
            children[node, 1] = gamma + 1
            todo.append((gamma + 1, gamma + 1, b))
    return children, ranges


def build(indices, pos):
    """indices u32 [T, 3] and the float rows of the positions [U, 3] of a render build -> the seven buffers, "summary" and "ranges"
    (the leaves every node covers)"""
    indices = np.asarray(indices, np.uint32).reshape(-1, 3)
    pos = np.ascontiguousarray(pos, np.float32)
    T = len(indices)
    tri_pos = pos[indices] if T else np.zeros((0, 3, 3), np.float32)
    live = np.isfinite(tri_pos).all(axis=(1, 2))
    t_live = np.flatnonzero(live).astype(np.uint32)
    L = len(t_live)
    p = tri_pos[t_live]
    box = np.concatenate([least(p, 1), greatest(p, 1)], axis=1).reshape(L, 6)
    if L:
        lo, hi = least(box[:, :3], 0), greatest(box[:, 3:], 0)
    else:
        lo, hi = np.full(3, np.inf, np.float32), np.full(3, -np.inf, np.float32)
    code = codes_of(p, lo, hi) if L else np.zeros(0, np.uint32)
    order = np.lexsort((t_live, code))
    out = {"leaf_tri": t_live[order], "leaf_code": code[order].astype(np.uint32), "leaf_box": box[order],
           "leaf_positions": p[order].reshape(L, 9), "scene_box": np.concatenate([lo, hi]).reshape(1, 6).astype(np.float32)}
    children, ranges = tree_of(out["leaf_code"])
    node_box = np.zeros((len(children), 6), np.float32)
    height = np.zeros(len(children), np.int64)
    for node in np.argsort(ranges[:, 1] - ranges[:, 0], kind="stable") if len(children) else []:   # children before parents
        rows, h = [], 0
        for c in children[node]:
            n = int(c & ~np.uint32(LEAF))
            rows.append(out["leaf_box"][n] if c & LEAF else node_box[n])
            h = max(h, 0 if c & LEAF else int(height[n]))
        rows = np.stack(rows)
        node_box[node] = np.concatenate([least(rows[:, :3], 0), greatest(rows[:, 3:], 0)])
        height[node] = h + 1
    out["node_children"], out["node_box"], out["ranges"] = children, node_box, ranges
    out["summary"] = (T, L, T - L, len(np.unique(code)), int(height[0]) if len(children) else 0)
    return out


def fan_triangles(degrees, corners):
    """the fan triangles (c_0, c_k, c_k+1) of every face, in face order: what a render build of a welded mesh calls "indices" """
    out, at = [], 0
    for d in np.asarray(degrees).tolist():
        c = corners[at:at + d]
        out += [[c[0], c[k], c[k + 1]] for k in range(1, d - 1)]
        at += d
    return np.array(out, np.uint32).reshape(-1, 3)


def of_arrays(pos, degrees, corners):
    return build(fan_triangles(degrees, np.asarray(corners, np.uint32)), np.asarray(pos, np.float32))


def ray_set(bvh, n, seed):
    """n rays about the hierarchy's scene, float32 (origins [n, 3], dirs [n, 3]): a third random -- from a sphere about the scene
    towards a point of its box grown by a half --, a third aimed exactly at a corner of a leaf from there, a third parallel to an
    axis from a face of the scene box, the other two coordinates a leaf corner's or random, the zero components -0 on odd rays"""
    rng = np.random.default_rng(seed)
    box = bvh["scene_box"][0].astype(np.float64)
    if not len(bvh["leaf_tri"]):
        box = np.array([0.0, 0, 0, 1, 1, 1])
    lo, hi = box[:3], box[3:]
    mid, half = (lo + hi) / 2, np.maximum((hi - lo) / 2, 1e-3)
    radius = 2.5 * np.linalg.norm(half)
    corners = bvh["leaf_positions"].reshape(-1, 3) if len(bvh["leaf_tri"]) else np.zeros((1, 3), np.float32)
    third = n // 3

    def sphere(k):
        v = rng.normal(size=(k, 3))
        return (mid + radius * v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)

    o0 = sphere(third)
    d0 = ((mid + 1.5 * half * rng.uniform(-1, 1, (third, 3))).astype(np.float32) - o0).astype(np.float32)
    o1 = sphere(third)
    d1 = (corners[rng.integers(0, len(corners), third)] - o1).astype(np.float32)
    k = n - 2 * third
    axis, sign = rng.integers(0, 3, k), rng.integers(0, 2, k) * 2 - 1
    o2 = np.where(rng.integers(0, 2, (k, 1)) == 1, corners[rng.integers(0, len(corners), k)],
                  (mid + 1.2 * half * rng.uniform(-1, 1, (k, 3)))).astype(np.float32)
    rows = np.arange(k)
    o2[rows, axis] = np.where(sign > 0, lo[axis], hi[axis]).astype(np.float32)
    d2 = np.zeros((k, 3), np.float32)
    d2[1::2] = -0.0
    d2[rows, axis] = sign
    return np.concatenate([o0, o1, o2]), np.concatenate([d0, d1, d2])


# ---- the cast
def valid_rays(O, D):
    return np.isfinite(O).all(axis=1) & np.isfinite(D).all(axis=1) & (D != 0).any(axis=1)


def interval(box, O, D, tmin, tmax):
    """box f32 [m, 6] against rays O, D f64 [n, 3] (valid ones) -> (passes, near, far) [n, m]"""
    lo, hi = box[None, :, :3].astype(np.float64), box[None, :, 3:].astype(np.float64)
    o, d = O[:, None, :], D[:, None, :]
    with np.errstate(all="ignore"):
        inv = 1.0 / d
        a, c = (lo - o) * inv, (hi - o) * inv
    flat = d == 0
    outside = (flat & ((o < lo) | (o > hi))).any(axis=2)
    n = np.where(flat, -np.inf, np.minimum(a, c)).max(axis=2)
    f = np.where(flat, np.inf, np.maximum(a, c)).min(axis=2)
    n1, f1 = n - np.abs(n) * WIDEN, f + np.abs(f) * WIDEN
    near, far = np.maximum(tmin, n1), np.minimum(tmax, f1)
    return ~outside & (near <= far), near, far


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def hits(leaf_positions, O, D, near, far):
    """the hit clause of every (ray, leaf): (accepted, tt, u, v) [n, m]"""
    P = leaf_positions.astype(np.float64).reshape(1, -1, 3, 3)
    o, d = O[:, None, :], D[:, None, :]
    with np.errstate(all="ignore"):
        e1, e2 = P[:, :, 1] - P[:, :, 0], P[:, :, 2] - P[:, :, 0]
        p = cross(d, e2)
        det = dot(e1, p)
        s = o - P[:, :, 0]
        q = cross(s, e1)
        u, v, tt = dot(s, p) / det, dot(d, q) / det, dot(e2, q) / det
        ok = np.isfinite(det) & (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (near <= tt) & (tt <= far)
    return ok, tt, u, v


def cast(bvh, origins, dirs, tmin=0.0, tmax=np.inf, chunk=256):
    """every ray against every leaf -> {"tri" u32 [n], "t" f32 [n], "uv" f32 [n, 2], "hits": the rays that hit}"""
    origins, dirs = np.asarray(origins, np.float32).reshape(-1, 3), np.asarray(dirs, np.float32).reshape(-1, 3)
    n, L = len(dirs), len(bvh["leaf_tri"])
    if len(origins) == 1 and n != 1:
        origins = np.broadcast_to(origins, (n, 3))
    tri, t, uv = np.full(n, NO_ELEMENT, np.uint32), np.full(n, np.inf, np.float32), np.zeros((n, 2), np.float32)
    good = np.flatnonzero(valid_rays(origins, dirs)) if L else np.zeros(0, np.int64)
    for at in range(0, len(good), chunk):
        rows = good[at:at + chunk]
        O, D = origins[rows].astype(np.float64), dirs[rows].astype(np.float64)
        passes, near, far = interval(bvh["leaf_box"], O, D, tmin, tmax)
        ok, tt, u, v = hits(bvh["leaf_positions"], O, D, near, far)
        ok &= passes
        tt = np.where(ok, tt, np.inf)
        best = tt.min(axis=1)
        first = np.where(ok & (tt == best[:, None]), bvh["leaf_tri"][None, :].astype(np.int64), 1 << 40)
        leaf = first.argmin(axis=1)
        hit = ok.any(axis=1)
        k = np.arange(len(rows))
        tri[rows[hit]] = bvh["leaf_tri"][leaf[hit]]
        with np.errstate(over="ignore"):
            t[rows[hit]] = tt[k, leaf][hit].astype(np.float32)   # the winner's own tt: among equal ones a -0 and a +0 differ in bits
            uv[rows[hit]] = np.stack([u[k, leaf], v[k, leaf]], axis=1)[hit].astype(np.float32)
    return {"tri": tri, "t": t, "uv": uv, "hits": int((tri != NO_ELEMENT).sum())}


def walk(bvh, origin, direction, tmin=0.0, tmax=np.inf):
    """one ray down the tree with a stack, the nearer child first, skipping a node whose box fails or whose near is greater than the
    best tt so far -> (tri, t, u, v, box tests made)"""
    O, D = np.asarray(origin, np.float32).astype(np.float64).reshape(1, 3), np.asarray(direction, np.float32).astype(np.float64).reshape(1, 3)
    L = len(bvh["leaf_tri"])
    best, tests = (np.inf, NO_ELEMENT, 0.0, 0.0), 0
    if not L or not valid_rays(O, D)[0]:
        return (NO_ELEMENT, np.float32(np.inf), np.float32(0), np.float32(0), 0)

    def leaf(i, near, far):
        nonlocal best
        ok, tt, u, v = hits(bvh["leaf_positions"][i:i + 1], O, D, near, far)
        t = int(bvh["leaf_tri"][i])
        if ok[0, 0] and (tt[0, 0] < best[0] or (tt[0, 0] == best[0] and t < best[1])):
            best = (tt[0, 0], t, u[0, 0], v[0, 0])

    def box_of(c):
        nonlocal tests
        tests += 1
        n = int(c & ~np.uint32(LEAF))
        passes, near, far = interval((bvh["leaf_box"] if c & LEAF else bvh["node_box"])[n:n + 1], O, D, tmin, tmax)
        return n, bool(passes[0, 0]), near[0, 0], far[0, 0]

    if L == 1:
        n, passes, near, far = box_of(np.uint32(LEAF))
        if passes:
            leaf(0, near, far)
    stack = [(0, -np.inf)] if L > 1 else []
    deepest = 0
    while stack:
        deepest = max(deepest, len(stack))
        node, bound = stack.pop()
        if bound > best[0]:
            continue
        kids = []
        for c in bvh["node_children"][node]:
            n, passes, near, far = box_of(c)
            if passes and not near > best[0]:
                if c & LEAF:
                    leaf(n, near, far)
                else:
                    kids.append((n, near))
        kids = [k for k in kids if not k[1] > best[0]]
        kids.sort(key=lambda k: -k[1])   # the nearer one on top
        stack.extend(kids)
    assert deepest <= 64
    hit = best[1] != NO_ELEMENT
    return (best[1], np.float32(best[0]) if hit else np.float32(np.inf), np.float32(best[2]), np.float32(best[3]), tests)
