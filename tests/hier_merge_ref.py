"""Reference code shared by tests/test_hier_merge_cpu.py and tests/test_gpu_hier_merge.py: a recursive numpy
restatement of the chunk merger (include/hlgs.h, hlgs_hier_merge_*) written from that contract -- an
explicit tree with child lists, the splice by handing child lists upwards, the rows by a pre-order recursion -- the
same rows in closed form (the level-wise sums the GPU uses) as a second, independent function, and the seeded scenes.

A chunk is the tuple load_dynamic_hierarchy returns, as numpy arrays: pos (n, 3), shs (n, C, 3), alpha (n, 1),
log_scales (n, 3), rot (n, 4) float32 and nodes (n, 6) int32."""
import sys

import numpy as np

DEPTH, PARENT, CHILD_COUNT, FIRST_CHILD, NEXT_SIBLING, MAX_SIDE = range(6)
F = np.float32


# ---------------------------------------------------------------------------------------------- the restatement
def weights(pos, k, centers, falloff=0.05):
    """The weight of every row of chunk k (pos with row 0 already at the centre), float32, one rounding per operation.
    A NaN position gives NaN."""
    pos, c, f = np.asarray(pos, F), np.asarray(centers, F), F(falloff)

    def dist(j):
        d = pos - c[j]
        return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])

    with np.errstate(invalid="ignore", over="ignore"):
        dk = dist(k)
        m = np.full(len(pos), 1e12, F)
        for j in range(len(c)):
            if j != k:
                dj = dist(j)
                m = np.where(dj < m, dj, m)
        a = F(-1.0) / ((F(2.0) * f) * m)
        b = (F(1.0) + f) / (F(2.0) * f)
        w = np.where(dk <= (F(1.0) - f) * m, F(1.0), np.where(dk > (F(1.0) + f) * m, F(0.0), a * dk + b))
    return w.astype(F)


class _Node:
    __slots__ = ("row", "w", "kids", "was_leaf")


def _children(nodes, i):
    out, c = [], int(nodes[i, FIRST_CHILD])
    for _ in range(int(nodes[i, CHILD_COUNT])):
        out.append(c)
        c = int(nodes[c, NEXT_SIBLING])
    return out


def _load(nodes, w, i):
    nd = _Node()
    nd.row, nd.w, nd.was_leaf = i, w[i], nodes[i, CHILD_COUNT] == 0
    nd.kids = [_load(nodes, w, c) for c in _children(nodes, i)]
    return nd


def _filter(nd):
    """The kept nodes that take nd's place in its parent's child list: nd itself, or its spliced descendants."""
    kids = []
    for c in nd.kids:
        kids += _filter(c)
    if nd.w > 0:
        nd.kids = kids
        return [nd]
    return kids


def _populate(nd, parent, depth, rows, src, leaf_rank):
    me = len(rows)
    rank = -1
    if nd.was_leaf:
        rank = leaf_rank[0]
        leaf_rank[0] += 1
    rows.append([depth, parent, len(nd.kids), me + 1, 0, rank])
    src.append(nd)
    prev = None
    for c in nd.kids:
        cid = _populate(c, me, depth + 1, rows, src, leaf_rank)
        if prev is not None:
            rows[prev][NEXT_SIBLING] = cid
        prev = cid
    return me


def flat(chunk):
    pos, shs, alpha, ls, rot, nodes = [np.asarray(a) for a in chunk]
    n = len(pos)
    return (pos.astype(F), shs.astype(F).reshape(n, -1), alpha.astype(F).reshape(n), ls.astype(F), rot.astype(F),
            nodes.astype(np.int32))


def merge_ref(chunks, centers, falloff=0.05, root_scale=1e4):
    """dict(pos, shs (G, C3), alpha (G,), log_scales, rot, nodes, chunk_roots): the merged hierarchy, recursively."""
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 20000))
    centers = np.asarray(centers, F)
    K = len(chunks)
    rows = [[0, -1, K, 1, 0, -1]]
    cols = {k: [None] for k in ("pos", "shs", "alpha", "log_scales", "rot")}
    leaf_rank, roots = [0], []
    for k, ch in enumerate(chunks):
        pos, shs, alpha, ls, rot, nodes = flat(ch)
        pos = pos.copy()
        pos[0] = centers[k]
        w = weights(pos, k, centers, falloff)
        top = _filter(_load(nodes, w, 0))
        if not (w[0] > 0):
            raise ValueError("chunk root dropped")
        src = []
        rid = _populate(top[0], 0, 1, rows, src, leaf_rank)
        if roots:
            rows[roots[-1]][NEXT_SIBLING] = rid
        roots.append(rid)
        idx = np.array([nd.row for nd in src])
        cols["pos"].append(pos[idx])
        cols["shs"].append(shs[idx])
        cols["alpha"].append(alpha[idx] * w[idx])
        cols["log_scales"].append(ls[idx])
        cols["rot"].append(rot[idx])
    nodes = np.array(rows, np.int32)
    a = np.array([cols["alpha"][k + 1][0] for k in range(K)], np.float64)
    num, den, sh = np.zeros(3), 0.0, np.zeros(cols["shs"][1].shape[1])
    for k in range(K):  # chunk order, float64, rounded once
        num = num + a[k] * centers[k].astype(np.float64)
        den = den + a[k]
        sh = sh + cols["shs"][k + 1][0].astype(np.float64)
    cols["pos"][0] = (num / max(den, 1e-12)).astype(F)[None]
    cols["shs"][0] = (sh / float(K)).astype(F)[None]
    cols["alpha"][0] = np.array([max(F(x) for x in a)], F)
    cols["log_scales"][0] = np.full((1, 3), F(np.log(np.float64(F(root_scale)))), F)
    cols["rot"][0] = np.array([[1, 0, 0, 0]], F)
    out = {k: np.concatenate(v) for k, v in cols.items()}
    out["nodes"] = nodes
    out["chunk_roots"] = np.array(roots, np.int32)
    return out


def closed_form_nodes(chunks, centers, falloff=0.05):
    """(nodes, chunk_roots, src) of the merge without recursion: s = kept nodes and l = kept input-leaves per input
    subtree and t = spliced children, bottom-up by depth; base, leaf base, new parent, new depth and end handed from
    parent to children top-down; every kept row then in closed form.  src[id] = (chunk, input row), (-1, -1) for
    row 0."""
    centers = np.asarray(centers, F)
    K = len(chunks)
    st = []
    for k, ch in enumerate(chunks):
        pos, _, _, _, _, nodes = flat(ch)
        pos = pos.copy()
        pos[0] = centers[k]
        keep = (weights(pos, k, centers, falloff) > 0).astype(np.int64)
        n = len(nodes)
        by_depth = np.argsort(nodes[:, DEPTH], kind="stable")
        s, l, t = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
        for i in by_depth[::-1]:
            kids = _children(nodes, i)
            s[i] = keep[i] + sum(s[c] for c in kids)
            l[i] = (keep[i] and nodes[i, CHILD_COUNT] == 0) + sum(l[c] for c in kids)
            t[i] = sum(1 if keep[c] else t[c] for c in kids)
        st.append((nodes, keep, by_depth, s, l, t))
    G = 1 + sum(int(x[3][0]) for x in st)
    out = np.zeros((G, 6), np.int32)
    out[0] = (0, -1, K, 1, 0, -1)
    src = np.full((G, 2), -1, np.int64)
    off, loff, roots = 1, 0, []
    for k, (nodes, keep, by_depth, s, l, t) in enumerate(st):
        n = len(nodes)
        base, lbase, npar, ndep, end = (np.zeros(n, np.int64) for _ in range(5))
        base[0], lbase[0], npar[0], ndep[0] = off, loff, 0, 1
        end[0] = off + s[0] if k == K - 1 else -1
        for i in by_depth:
            b, kp = base[i], keep[i]
            if kp:
                after = b + s[i]
                out[b] = (ndep[i], npar[i], t[i], b + 1, 0 if after == end[i] else after,
                          lbase[i] if nodes[i, CHILD_COUNT] == 0 else -1)
                src[b] = (k, i)
            cb, clb = b + kp, lbase[i]
            for c in _children(nodes, i):
                base[c], lbase[c] = cb, clb
                npar[c] = b if kp else npar[i]
                ndep[c] = ndep[i] + kp
                end[c] = b + s[i] if kp else end[i]
                cb += s[c]
                clb += l[c]
        roots.append(off)
        off += int(s[0])
        loff += int(l[0])
    return out, np.array(roots, np.int32), src


def splice_stats(chunk, k, centers, falloff=0.05):
    """What a scene exercises, from the restatement alone: the fractions of rows with w = 1, 0 < w < 1 and w = 0, the
    dropped interior rows with a kept descendant, and the largest child count after splicing."""
    pos, _, _, _, _, nodes = flat(chunk)
    pos = pos.copy()
    pos[0] = np.asarray(centers, F)[k]
    w = weights(pos, k, centers, falloff)
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 20000))
    root = _load(nodes, w, 0)
    splices = [0]

    def kept_below(nd):
        below = sum([kept_below(c) for c in nd.kids])
        if not nd.w > 0 and nd.kids and below > 0:
            splices[0] += 1
        return below + (1 if nd.w > 0 else 0)

    kept_below(root)
    top = _filter(root)
    widest = [0]

    def walk(nd):
        widest[0] = max(widest[0], len(nd.kids))
        for c in nd.kids:
            walk(c)

    walk(top[0])
    n = float(len(w))
    return dict(one=np.sum(w == 1) / n, band=np.sum((w > 0) & (w < 1)) / n, zero=np.sum(~(w > 0)) / n,
                splices=splices[0], widest=widest[0])


# ---------------------------------------------------------------------------------------------- scenes
def centers_for(K):
    """Chunk centres 4 apart: the issue's triangle for K <= 3, the corners of a cube of side 4 beyond."""
    if K <= 3:
        return np.array([(0, 0, 0), (4, 0, 0), (2, 3.5, 0)], F)[:K]
    return np.array([(4 * (j & 1), 4 * ((j >> 1) & 1), 4 * ((j >> 2) & 1)) for j in range(K)], F)


def _rows(n, shf, rng):
    """Random trained-looking values for everything but the position and the links."""
    shs = rng.normal(0, 0.5, (n, shf // 3, 3) if shf % 3 == 0 else (n, shf)).astype(F)
    alpha = rng.uniform(0.05, 1.0, (n, 1)).astype(F)
    ls = rng.uniform(-5.0, -1.0, (n, 3)).astype(F)
    rot = rng.normal(0, 1, (n, 4)).astype(F)
    return shs, alpha, ls, rot


def tree_over(leaves, shf, rng):
    """A median-split binary tree over the leaf positions, rows in pre-order, every interior position the mean of its
    children's (float32)."""
    leaves = np.asarray(leaves, F)
    L = len(leaves)
    n = 2 * L - 1
    pos = np.zeros((n, 3), F)
    nodes = np.zeros((n, 6), np.int32)
    nxt = [0]
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 20000))

    def build(idx, parent, depth):
        me = nxt[0]
        nxt[0] += 1
        nodes[me] = (depth, parent, 0, 0, 0, 0)
        if len(idx) == 1:
            pos[me] = leaves[idx[0]]
            return me
        p = leaves[idx]
        axis = int(np.argmax(p.max(0) - p.min(0)))
        order = idx[np.argsort(p[:, axis], kind="stable")]
        h = len(order) // 2
        a = build(order[:h], me, depth + 1)
        b = build(order[h:], me, depth + 1)
        nodes[me, CHILD_COUNT], nodes[me, FIRST_CHILD] = 2, a
        nodes[a, NEXT_SIBLING] = b
        pos[me] = (pos[a] + pos[b]) * F(0.5)
        return me

    build(np.arange(L), -1, 0)
    return (pos,) + _rows(n, shf, rng) + (nodes,)


def _cube(rng, L, center, half):
    return (np.asarray(center, F) + rng.uniform(-half, half, (L, 3))).astype(F)


def _on_ratio(rng, pts, c0, c1, lo=0.94, hi=1.06):
    """pts moved along the line c0 -> c1 until |p - c0| / |p - c1| is a ratio drawn uniformly from [lo, hi]."""
    c0, c1 = np.asarray(c0, np.float64), np.asarray(c1, np.float64)
    u = (c1 - c0) / np.linalg.norm(c1 - c0)
    p = np.asarray(pts, np.float64)
    perp = p - c0 - np.outer((p - c0) @ u, u)
    r = rng.uniform(lo, hi, len(p))
    span = np.linalg.norm(c1 - c0)
    a, b = np.full(len(p), -60.0), np.full(len(p), span)  # the ratio grows with the abscissa on (-inf, span]

    def ratio(x):
        q = c0 + perp + np.outer(x, u)
        return np.linalg.norm(q - c0, axis=1) / np.linalg.norm(q - c1, axis=1)

    # below the abscissa of the smallest ratio the function falls again: start from that minimum
    a = np.where(ratio(np.zeros(len(p))) < r, 0.0, a)
    for _ in range(60):
        mid = 0.5 * (a + b)
        up = ratio(mid) < r
        a, b = np.where(up, mid, a), np.where(up, b, mid)
    return (c0 + perp + np.outer(0.5 * (a + b), u)).astype(F)


def permuted(chunk, new_of):
    """The same tree with old row i stored at row new_of[i] (new_of[0] = 0) and every link remapped (first_child of a
    leaf stays as it is)."""
    pos, shs, alpha, ls, rot, nodes = chunk
    new_of = np.asarray(new_of, np.int64)
    old_of = np.argsort(new_of)
    nd = nodes[old_of].copy()
    nd[1:, PARENT] = new_of[nd[1:, PARENT]]
    inner = nd[:, CHILD_COUNT] > 0
    nd[inner, FIRST_CHILD] = new_of[nd[inner, FIRST_CHILD]]
    link = nd[:, NEXT_SIBLING] > 0
    nd[link, NEXT_SIBLING] = new_of[nd[link, NEXT_SIBLING]]
    return pos[old_of], shs[old_of], alpha[old_of], ls[old_of], rot[old_of], nd.astype(np.int32)


def shuffled(chunk, seed=0):
    """permuted() with rows 1 .. n-1 in a seeded random order."""
    n = len(chunk[0])
    rng = np.random.default_rng(1000 + seed)
    return permuted(chunk, np.concatenate([[0], 1 + rng.permutation(n - 1)]))


def middle_swapped(chunk, phase):
    """permuted() with rows j and j + 1 exchanged for every j = phase (mod 4), j >= 1: of four consecutive rows the
    outer two stay and the inner two trade places, so a copy that compares only the ends of a run goes wrong."""
    n = len(chunk[0])
    new_of = np.arange(n)
    for j in range(phase if phase >= 1 else 4, n - 1, 4):
        new_of[j], new_of[j + 1] = j + 1, j
    return permuted(chunk, new_of)


def appended(chunk, seed=0, fraction=0.05):
    """5 % of the leaves given two children each, appended behind the last row as hlgs_core.mcmc.apply_spawn writes
    them: zero rows but for depth, parent and the first one's next_sibling."""
    pos, shs, alpha, ls, rot, nodes = chunk
    n = len(pos)
    rng = np.random.default_rng(2000 + seed)
    leaves = np.where(nodes[:, CHILD_COUNT] == 0)[0]
    leaves = leaves[leaves > 0]
    add = np.sort(rng.choice(leaves, max(1, int(fraction * len(leaves))), replace=False)) if len(leaves) else leaves
    m = len(add)
    nd = np.concatenate([nodes, np.zeros((2 * m, 6), np.int32)])
    first = n + 2 * np.arange(m)
    nd[add, CHILD_COUNT], nd[add, FIRST_CHILD] = 2, first
    nd[first, DEPTH] = nd[first + 1, DEPTH] = nd[add, DEPTH] + 1
    nd[first, PARENT] = nd[first + 1, PARENT] = add
    nd[first, NEXT_SIBLING] = first + 1
    rep = np.repeat(add, 2)
    jitter = rng.normal(0, 0.3, (2 * m, 3)).astype(F)
    cat = lambda a, extra: np.concatenate([a, extra])  # noqa: E731
    return (cat(pos, pos[rep] + jitter), cat(shs, shs[rep]), cat(alpha, alpha[rep] * F(0.5)), cat(ls, ls[rep]),
            cat(rot, rot[rep]), nd.astype(np.int32))


def make_chunk(kind, L, k, K, shf=3, seed=0):
    """Chunk k of K of a scene kind with L leaves (chain: L levels; wide: L children)."""
    rng = np.random.default_rng([seed, k, K, L])
    cen = centers_for(K)
    c = cen[k]
    if kind == "uniform":
        return tree_over(_cube(rng, L, c, 3.2), shf, rng)
    if kind == "bisector":
        pts = _cube(rng, L, c, 3.2)
        if K > 1:
            other = cen[(k + 1) % K]
            pts[: L // 2] = _on_ratio(rng, pts[: L // 2], c, other)
        return tree_over(pts, shf, rng)
    if kind == "all_far":
        return tree_over(_cube(rng, L, cen[(k + 1) % K], 1.0), shf, rng)
    if kind == "chain":
        n = 2 * L + 1
        nodes = np.zeros((n, 6), np.int32)
        for d in range(L):  # interior row 2 d: a leaf child 2 d + 1, then the next interior row (or a last leaf)
            i = 2 * d
            nodes[i, CHILD_COUNT], nodes[i, FIRST_CHILD] = 2, i + 1
            nodes[i + 1] = (d + 1, i, 0, 0, i + 2, 0)
            nodes[i + 2, DEPTH], nodes[i + 2, PARENT] = d + 1, i
        nodes[0, PARENT] = -1
        return (_cube(rng, n, c, 3.2),) + _rows(n, shf, rng) + (nodes,)
    if kind == "wide":
        n = L + 1
        nodes = np.zeros((n, 6), np.int32)
        nodes[0] = (0, -1, L, 1, 0, 0)
        for i in range(1, n):
            nodes[i] = (1, 0, 0, 0, i + 1 if i + 1 < n else 0, 0)
        return (_cube(rng, n, c, 3.2),) + _rows(n, shf, rng) + (nodes,)
    if kind == "appended":
        return appended(tree_over(_cube(rng, L, c, 3.2), shf, rng), seed=seed + k)
    raise ValueError(kind)


def make_scene(kind, L, K, shf=3, seed=0, shuffle=False):
    """(chunks, centers) of K chunks; L an int or one leaf count per chunk."""
    Ls = [L] * K if np.isscalar(L) else list(L)
    chunks = [make_chunk(kind, Ls[k], k, K, shf, seed) for k in range(K)]
    if shuffle:
        chunks = [shuffled(ch, seed + k) for k, ch in enumerate(chunks)]
    return chunks, centers_for(K)
