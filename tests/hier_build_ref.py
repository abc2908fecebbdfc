"""Reference code shared by tests/test_hier_build_cpu.py and tests/test_gpu_hier_build.py: a recursive numpy
restatement of the hierarchy creator (submodules/gaussianhierarchy: PointbasedKdTreeGenerator.cpp:16-68,
ClusterMerger.cpp:23-141, rotation_aligner.cpp:23-115, writer.cpp:99-204) as include/hlgs.h states it for
hlgs_hier_build, the creator's filter (mainHierarchyCreator.cpp:87-152), the node table in closed form, and the seeded
scenes of the tests.

build_ref(scene, dtype) runs the kd-tree in float32 always (the tree is part of the contract) and the merge and the
alignment in `dtype`: np.float32 rounds every operation on its own, in the order the reference writes them; np.float64
is the yardstick both the float32 restatement and the GPU are measured against.  The symmetric eigen-decomposition is
numpy's (LAPACK syevd) at that precision.
"""
import sys

import numpy as np

DEPTH, PARENT, CHILD_COUNT, FIRST_CHILD, NEXT_SIBLING, MAX_SIDE = range(6)
EPS32 = float(np.finfo(np.float32).eps)


# ------------------------------------------------------------------ small matrices
def matrix_from_quat(q):
    """common.h:103-117, q = (s, x, y, z), in q's dtype."""
    T = q.dtype.type
    s, x, y, z = q
    one, two = T(1), T(2)
    return np.array([[one - two * (y * y + z * z), two * (x * y - s * z), two * (x * z + s * y)],
                     [two * (x * y + s * z), one - two * (x * x + z * z), two * (y * z - s * x)],
                     [two * (x * z - s * y), two * (y * z + s * x), one - two * (x * x + y * y)]], dtype=q.dtype)


def quat_from_matrix(m):
    """Eigen::Quaternion(Matrix3) as (w, x, y, z), in m's dtype."""
    T = m.dtype.type
    half, one = T(0.5), T(1)
    q = np.zeros(4, m.dtype)
    t = (m[0, 0] + m[1, 1]) + m[2, 2]
    if t > 0:
        t = np.sqrt(t + one)
        q[0] = half * t
        t = half / t
        q[1] = (m[2, 1] - m[1, 2]) * t
        q[2] = (m[0, 2] - m[2, 0]) * t
        q[3] = (m[1, 0] - m[0, 1]) * t
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = np.sqrt(((m[i, i] - m[j, j]) - m[k, k]) + one)
        q[1 + i] = half * t
        t = half / t
        q[0] = (m[k, j] - m[j, k]) * t
        q[1 + j] = (m[j, i] + m[i, j]) * t
        q[1 + k] = (m[k, i] + m[i, k]) * t
    return q


def col_det(m):
    """c0.cross(c1).dot(c2) of the columns."""
    cx = m[1, 0] * m[2, 1] - m[2, 0] * m[1, 1]
    cy = m[2, 0] * m[0, 1] - m[0, 0] * m[2, 1]
    cz = m[0, 0] * m[1, 1] - m[1, 0] * m[0, 1]
    return (cx * m[0, 2] + cy * m[1, 2]) + cz * m[2, 2]


def covariance_of(s, q):
    """common.h:119-146 as six entries (xx, xy, xz, yy, yz, zz), sums left to right."""
    t = matrix_from_quat(q) * s[None, :]
    return np.array([(t[i, 0] * t[j, 0] + t[i, 1] * t[j, 1]) + t[i, 2] * t[j, 2]
                     for i in range(3) for j in range(i, 3)], dtype=s.dtype)


def surface(s):
    return (s[0] * s[1] + s[0] * s[2]) + s[1] * s[2]


def normalise(q):
    return q / np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])


def sym(c):
    return np.array([[c[0], c[1], c[2]], [c[1], c[3], c[4]], [c[2], c[4], c[5]]], dtype=c.dtype)


# ------------------------------------------------------------------ the creator, recursively
class TreeNode:
    __slots__ = ("children", "leaf", "g")

    def __init__(self):
        self.children, self.leaf, self.g = [], -1, None


def kd_tree(xyz, scales, idx):
    """PointbasedKdTreeGenerator.cpp:16-68 in float32 over the rows idx; ties by (position[axis], row)."""
    node = TreeNode()
    num = len(idx)
    if num == 1:
        node.leaf = int(idx[0])
        return node
    r = np.float32(3.0) * scales[idx].max(axis=1)
    lo = (xyz[idx] - r[:, None]).min(axis=0)
    hi = (xyz[idx] + r[:, None]).max(axis=0)
    axis, greatest = 0, np.float32(0)
    for a in range(3):
        dist = hi[a] - lo[a]
        if dist > greatest:
            greatest, axis = dist, a
    order = idx[np.lexsort((idx, xyz[idx, axis]))]  # floats compare, so -0.0 ties with +0.0; then the row
    nl = num // 2
    node.children = [kd_tree(xyz, scales, order[:nl]), kd_tree(xyz, scales, order[nl:])]
    return node


def _gaussian(node, leaves):
    return leaves[node.leaf] if node.leaf >= 0 else node.g


def merge(node, leaves, T):
    """ClusterMerger.cpp:23-141: node.g = dict(pos, sh, op, scale, rot, cov) of every interior node, bottom-up."""
    if node.leaf >= 0:
        return
    for c in node.children:
        merge(c, leaves, T)
    gs = [_gaussian(c, leaves) for c in node.children]
    w = [g["op"] * surface(g["scale"]) for g in gs]
    W = (T(0) + w[0]) + w[1]
    with np.errstate(all="ignore"):
        a = [w[0] / W, w[1] / W]
        pos = (T(0) + a[0] * gs[0]["pos"]) + a[1] * gs[1]["pos"]
        sh = (T(0) + a[0] * gs[0]["sh"]) + a[1] * gs[1]["sh"]
        cov = np.zeros(6, T)
        for g, ai in zip(gs, a):
            d = g["pos"] - pos
            dd = np.array([d[0] * d[0], d[1] * d[0], d[2] * d[0], d[1] * d[1], d[2] * d[1], d[2] * d[2]], T)
            cov = cov + ai * (g["cov"] + dd)
        m = sym(cov)
        if np.isnan(m).any():
            raise RuntimeError("Found Nans!")
        ev, vec = np.linalg.eigh(m)
        if np.isnan(ev).any():
            raise RuntimeError("Found Nans!")
        while (ev == 0).any():
            for i in range(3):
                m[i, i] += max(m[i, i] * T(0.0001), T(EPS32))
            ev, vec = np.linalg.eigh(m)
        vec = vec.astype(T)
        if col_det(vec) < 0:
            vec[:, 2] = -vec[:, 2]
        scale = np.sqrt(np.abs(ev)).astype(T)
        node.g = dict(pos=pos, sh=sh, op=W / surface(scale), scale=scale, rot=quat_from_matrix(vec), cov=cov)


# the 48 signed column permutations in the reference's loop order (i, j, k, state)
CANDIDATES = [((i, j, 3 - i - j), state) for i in range(3) for j in range(3) if j != i for state in range(8)]
CAND_COLS = np.array([p for p, _ in CANDIDATES])
CAND_SIGN = np.array([[-1 if state & (1 << w) else 1 for w in range(3)] for _, state in CANDIDATES])


def best_candidate(Rm, Rref):
    """rotation_aligner.cpp:33-80: (i, j, k, matrix) of the first of the 24 proper signed column permutations of Rm
    with the strictly greatest sum(test * Rref) above 0, or None.  All candidates at once; every score is summed in
    the order of frobenius() (:14-21)."""
    T = Rm.dtype
    tests = Rm[:, CAND_COLS].transpose(1, 0, 2) * CAND_SIGN.astype(T)[:, None, :]  # (48, 3, 3)
    m = tests.transpose(1, 2, 0)  # m[r, c] over the candidates
    score = np.zeros(len(CANDIDATES), T)
    for r in range(3):
        for c in range(3):
            score = score + m[r, c] * Rref[r, c]
    with np.errstate(invalid="ignore"):
        score = np.where(col_det(m) < 0, -np.inf, score)
        best = int(np.argmax(score))  # the first of the greatest
        if not score[best] > 0:
            return None
    return (*CANDIDATES[best][0], tests[best])


def align(node, leaves):
    """rotation_aligner.cpp:90-110, top-down."""
    if node.leaf >= 0:
        return
    Rref = matrix_from_quat(node.g["rot"])
    for c in node.children:
        g = _gaussian(c, leaves)
        best = best_candidate(matrix_from_quat(g["rot"]), Rref)
        if best is not None:
            i, j, k, test = best
            g["rot"] = quat_from_matrix(test)
            g["scale"] = g["scale"][[i, j, k]]
        align(c, leaves)


def flatten(root, leaves, T):
    """writer.cpp:99-204: pre-order rows and the node table, by the writer's recursion."""
    rows, nodes = [], [[0, -1, 0, 0, 0, 0]]

    def rec(node, nid, depth):
        g = _gaussian(node, leaves)
        rows.append(g)
        nodes[nid][MAX_SIDE] = node.leaf if node.leaf >= 0 else -1
        nodes[nid][FIRST_CHILD] = len(nodes)
        nodes[nid][CHILD_COUNT] = len(node.children)
        nodes[nid][DEPTH] = depth
        for n, c in enumerate(node.children):
            nodes.append([0, nid, 0, 0, 0, 0])
            cid = len(nodes) - 1
            rec(c, cid, depth + 1)
            nodes[cid][NEXT_SIBLING] = len(nodes) if n < len(node.children) - 1 else 0

    rec(root, 0, 0)
    with np.errstate(all="ignore"):
        out = dict(pos=np.stack([g["pos"] for g in rows]), shs=np.stack([g["sh"] for g in rows]),
                   alpha=np.array([g["op"] for g in rows], T), scale=np.stack([g["scale"] for g in rows]),
                   rot=np.stack([g["rot"] for g in rows]), cov=np.stack([g["cov"] for g in rows]))
        out["log_scales"] = np.log(out["scale"])
    out["nodes"] = np.array(nodes, np.int32)
    return out


def build_ref(scene, dtype=np.float32):
    """The hierarchy of scene = dict(xyz, shs (N, F), opacity (N,), scales, rotations) float32 arrays.  Returns a
    dict of G = 2N - 1 pre-order rows: pos, shs, alpha, scale (activated), log_scales, rot, cov (the accumulated
    covariance, six entries) in `dtype`, and nodes (G, 6) int32."""
    T = np.dtype(dtype).type
    N = scene["xyz"].shape[0]
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 10000))
    root = kd_tree(scene["xyz"], scene["scales"], np.arange(N))
    leaves = []
    for i in range(N):
        s = scene["scales"][i].astype(T)
        q = normalise(scene["rotations"][i].astype(T))
        leaves.append(dict(pos=scene["xyz"][i].astype(T), sh=scene["shs"][i].astype(T), op=T(scene["opacity"][i]),
                           scale=s, rot=q, cov=covariance_of(s, q)))
    merge(root, leaves, T)
    align(root, leaves)
    return flatten(root, leaves, T)


def closed_form_nodes(N):
    """The five data-independent node columns (MAX_SIDE: 0 for a leaf, -1 else) from N alone, one node at a time, as
    k_hb_nodes walks them: a node of num leaves has num // 2 on its left, its left child at id + 1, its right child at
    id + 2 (num // 2).  Also returns the leaf position (from the left) of every leaf row, -1 for interior rows."""
    G = 2 * N - 1
    nodes = np.zeros((G, 6), np.int32)
    leafpos = np.full(G, -1, np.int64)
    for nid in range(G):
        cur, lo, num, depth, parent, sibling = 0, 0, N, 0, -1, 0
        while cur != nid:
            nl = num // 2
            parent = cur
            if nid < cur + 2 * nl:
                sibling, cur, num = cur + 2 * nl, cur + 1, nl
            else:
                sibling, cur, lo, num = 0, cur + 2 * nl, lo + nl, num - nl
            depth += 1
        nodes[nid] = [depth, parent, 2 if num > 1 else 0, nid + 1, sibling, -1 if num > 1 else 0]
        if num == 1:
            leafpos[nid] = lo
    return nodes, leafpos


def valid_mask_ref(scene):
    """mainHierarchyCreator.cpp:87-152."""
    o = scene["opacity"].reshape(-1)
    with np.errstate(invalid="ignore"):
        bad = np.isinf(o) | np.isnan(o) | (o == 0) | (scene["scales"] > 10).any(axis=1)
    for k in ("scales", "rotations", "xyz", "shs"):
        bad |= np.isnan(scene[k].reshape(len(o), -1)).any(axis=1)
    return ~bad


def rebuilt_cov(rot, log_scales):
    """R diag(exp(log_scales))^2 R^T in float64 from stored rows, (n, 3, 3)."""
    q = np.asarray(rot, np.float64)
    s2 = np.exp(np.asarray(log_scales, np.float64)) ** 2
    R = matrix_from_quat(q.T).transpose(2, 0, 1)  # all rows at once
    return np.einsum("nij,nj,nkj->nik", R, s2, R)


# ------------------------------------------------------------------ scenes
def _scene(xyz, rng, sh_floats, scale_lo=1e-3, scale_hi=1.0):
    n = xyz.shape[0]
    f = np.float32
    return dict(xyz=np.ascontiguousarray(xyz, f),
                shs=rng.normal(size=(n, sh_floats)).astype(f),
                opacity=rng.uniform(0.01, 1.0, size=n).astype(f),
                scales=np.exp(rng.uniform(np.log(scale_lo), np.log(scale_hi), size=(n, 3))).astype(f),
                rotations=(rng.normal(size=(n, 4)) * rng.uniform(0.2, 5.0, size=(n, 1))).astype(f))


def make_scene(kind, n, sh_floats=48, seed=0):
    """random: anisotropic scales 1e-3..1, unnormalised quaternions, opacity 0.01..1, positions in a 10-unit box.
    grid: positions on the integer grid {-1, 0, 1, 2}^2 x {0, 1} with one scale everywhere (many coordinate ties, equal
          x and y extents) and every zero of the first half of the rows written as -0.0.
    same: all positions identical.   plane: z = 0.25 for every row.
    far: scales 1e-6 in a unit box 1e3 from the origin."""
    rng = np.random.default_rng([seed, n, sh_floats, sorted(("random", "grid", "same", "plane", "far")).index(kind)])
    if kind == "random":
        return _scene(rng.uniform(-5, 5, size=(n, 3)), rng, sh_floats)
    if kind == "grid":
        xyz = np.stack([rng.integers(-1, 3, n), rng.integers(-1, 3, n), rng.integers(0, 2, n)], 1).astype(np.float32)
        half = xyz[:n // 2]
        half[half == 0] = -0.0
        sc = _scene(xyz, rng, sh_floats)
        sc["scales"][:] = np.float32(0.05)
        return sc
    if kind == "same":
        return _scene(np.tile(np.array([[0.5, -1.25, 3.0]]), (n, 1)), rng, sh_floats)
    if kind == "plane":
        xyz = rng.uniform(-5, 5, size=(n, 3))
        xyz[:, 2] = 0.25
        return _scene(xyz, rng, sh_floats)
    if kind == "far":
        xyz = np.array([600.0, -640.0, 480.0]) + rng.uniform(0, 1, size=(n, 3))
        return _scene(xyz, rng, sh_floats, 1e-6, 1e-6)
    raise ValueError(kind)
