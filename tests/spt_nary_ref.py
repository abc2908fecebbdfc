"""A numpy restatement of the n-ary contract of the SPT path (include/hlgs.h, "the n-ary contract").

TEST INFRASTRUCTURE ONLY.  Written from the contract, not from the library: per-level Python lists, float32
arithmetic with every operation rounded on its own, in the operation order oracle/spt_ref.py uses for the binary
case (prod(exp(scale)) as (e0 e1) e2; sqrt((s0 s1 + s0 s2) + s1 s2) / tg; distances as sqrt((dx^2 + dy^2) + dz^2)).

  children(nodes, v)                    the child list of row v: child_count members, first_child then next_sibling
  next_frontier(nodes, expanding)       rank-major: rank 0 of every expanding node in order, then rank 1, ...
  validate(nodes, root)                 contract 1 (ValueError on a violation)
  build_spt_nary(...)                   contract 2-6: the dict of build_hierarchical_spt, as numpy arrays, plus
                                        `frontiers` (the upper walk's levels), `cut`, `kept`/`dropped` candidate roots
  upper_tree_cut_nary(...)              the coarse cut over child lists; also returns the visited nodes' states
  order_nary(nodes)                     F*, level starts, preorder position and end, or None when not usable
"""
import numpy as np

from oracle import spt_ref as SR

F = np.float32
CC, FC, NS = 2, 3, 4


def children(nodes, v):
    out, m = [], int(nodes[v, FC])
    for _ in range(int(nodes[v, CC])):
        out.append(m)
        m = int(nodes[m, NS])
    return out


def next_frontier(nodes, expanding, with_parent=False):
    lists = [children(nodes, v) for v in expanding]
    out = []
    for r in range(max((len(c) for c in lists), default=0)):
        for i, c in enumerate(lists):
            if len(c) > r:
                out.append((c[r], i) if with_parent else c[r])
    return out


def validate(nodes, root):
    G = len(nodes)
    claimed = np.zeros(G, bool)
    for v in range(root, G):  # the rows before the root are skybox rows
        cc = int(nodes[v, CC])
        if cc < 0 or cc >= G:
            raise ValueError("child_count out of range")
        m = int(nodes[v, FC])
        for _ in range(cc):
            if m < root or m >= G:
                raise ValueError("member out of range")
            if m == root:
                raise ValueError("the root is a member")
            if claimed[m]:
                raise ValueError("a node in two lists")
            claimed[m] = True
            m = int(nodes[m, NS])


def _tables(nodes, scaling, tg):
    """Per node, each operation a float32 array operation of its own: prod(exp(scale)), 3 max(exp(scale)), and
    get_min_distance (-1e9 at leaves, at any level width)."""
    e = np.exp(np.asarray(scaling, F)).astype(F)
    vol = ((e[:, 0] * e[:, 1]).astype(F) * e[:, 2]).astype(F)
    r3 = (np.max(e, axis=1) * F(3.0)).astype(F)
    a, b, c = (e[:, 0] * e[:, 1]).astype(F), (e[:, 0] * e[:, 2]).astype(F), (e[:, 1] * e[:, 2]).astype(F)
    md = (np.sqrt(((a + b).astype(F) + c).astype(F)).astype(F) / F(tg)).astype(F)
    md[np.asarray(nodes)[:, CC] == 0] = F(-1000000000.0)
    return vol, r3, md


def _dist(a, b):
    d = (np.asarray(a, F) - np.asarray(b, F)).astype(F)
    q = (d * d).astype(F)
    return F(np.sqrt(F(F(q[0] + q[1]) + q[2])))


def build_spt_nary(nodes, xyz, scaling, root, volume, tg, min_size=100, use_bounding_spheres=True):
    nodes = np.asarray(nodes).astype(np.int64)
    xyz = np.asarray(xyz, F)
    scaling = np.asarray(scaling, F)
    validate(nodes, root)
    volume = F(volume)
    vol, r3, md = _tables(nodes, scaling, tg)
    # ---- contract 3: the upper walk
    stack, upper, cut, frontiers = [root], [], [], []
    while stack:
        frontiers.append(list(stack))
        upper += stack
        cut += [v for v in stack if nodes[v, CC] == 0]
        inner = [v for v in stack if nodes[v, CC] != 0]
        grow = [vol[v] > volume for v in inner]
        cut += [v for v, g in zip(inner, grow) if not g]
        stack = next_frontier(nodes, [v for v, g in zip(inner, grow) if g])
    # ---- contract 4: one SPT walk per inner node of the cut
    starts, smax, smin, gidx, roots, bsrs, dropped = [0], [], [], [], [], [], []
    spt_shapes = []
    for cn in cut:
        if nodes[cn, CC] == 0:
            continue
        centre = xyz[cn]
        ids, mins, maxs = [cn], [md[cn]], [F(1000000000000.0)]
        level, level_min = [cn], [mins[0]]
        bsr = r3[cn]
        while True:
            idx = [i for i, v in enumerate(level) if nodes[v, CC] > 0]
            nxt = next_frontier(nodes, [level[i] for i in idx], with_parent=True)
            if not nxt:
                break
            new_min = []
            for c, pi in nxt:
                cd = _dist(xyz[c], centre)
                bsr = max(bsr, F(cd + r3[c]))
                pmin = level_min[idx[pi]]
                m = F(md[c] + cd)
                new_min.append(m if m < pmin else pmin)
                ids.append(c)
                mins.append(new_min[-1])
                maxs.append(pmin)
            level, level_min = [c for c, _ in nxt], new_min
        if len(ids) > min_size:
            order = sorted(range(len(ids)), key=lambda i: -np.float64(maxs[i]))  # stable: ties in walk order
            smax += [maxs[i] for i in order]
            smin += [mins[i] for i in order]
            gidx += [ids[i] for i in order]
            starts.append(starts[-1] + len(ids))
            roots.append(cn)
            bsrs.append(bsr)
            spt_shapes.append(sorted({int(nodes[v, CC]) for v in ids}))
        else:
            upper += ids[1:]
            dropped.append(cn)
    # ---- contract 5: the upper-tree rows
    upper = sorted(upper)
    row_of = {v: i for i, v in enumerate(upper)}
    upper_a = np.asarray(upper)
    lb = lambda v: int(np.searchsorted(upper_a, v))  # noqa: E731
    U = len(upper)
    un = nodes[upper].copy()
    spt_of = {cn: k for k, cn in enumerate(roots)}
    for i, v in enumerate(upper):
        un[i, 5] = v
        un[i, 1] = lb(nodes[v, 1])
        if v in spt_of:
            un[i, 2], un[i, 3] = 0, spt_of[v]
        else:
            un[i, 3] = -1 if nodes[v, CC] == 0 else lb(nodes[v, FC])
        if nodes[v, NS] > 0:
            un[i, 4] = lb(nodes[v, NS])
    un[0, 1] = -1
    md2 = np.zeros(U, F)
    for i in range(U):
        m = md[int(un[un[i, 1], 5])]  # (row 0 reads the last row and is overwritten)
        md2[i] = F(m * m)
    md2[0] = F(1000000000000.0)
    # ---- contract 6: radii, children before parents (descending depth of the upper tree's own lists)
    radii = None
    if use_bounding_spheres:
        radii = np.zeros(U, F)
        order, frontier = [], [0]
        while frontier:
            order += frontier
            frontier = [c for v in frontier for c in children(un, v)]
        for i in reversed(order):
            v = upper[i]
            if v in spt_of:
                radii[i] = bsrs[spt_of[v]]
            elif un[i, CC] == 0:
                radii[i] = r3[v]
            else:
                radii[i] = max(F(radii[c] + _dist(xyz[upper[i]], xyz[upper[c]])) for c in children(un, i))
    assert all(v in row_of for v in roots)
    return dict(SPT_starts=np.array(starts, np.int32), SPT_max=np.array(smax, F), SPT_min=np.array(smin, F),
                SPT_gaussian_indices=np.array(gidx, np.int32), SPT_root_hierarchy_indices=np.array(roots, np.int32),
                upper_tree_nodes=un.astype(np.int32), upper_tree_xyz=xyz[upper], upper_tree_scaling=scaling[upper],
                min_distance_squared=md2, bounding_sphere_radii=radii,
                frontiers=frontiers, cut=cut, dropped=dropped, spt_child_counts=spt_shapes)


def upper_tree_cut_nary(nodes, xyz, bounds, md2, planes, cam, dmul=1.0, use_frustum=True, use_lod=True):
    """The coarse cut from root 0 over child lists (contract 2, 3); planes (4, 4) / cam (3,) for one view or (n, 4, 4)
    / (n, 3) for the union of n views, as oracle.spt_ref.upper_tree_cut.  Returns (cut, states, level sizes): states
    maps every visited node to 0 culled, 1 leaf, 2 condition false, 3 expand."""
    nodes = np.asarray(nodes)
    xyz = np.asarray(xyz, F)
    pls = None if planes is None else np.asarray(planes, F).reshape(-1, 4, 4)
    stack, cut, states, sizes = [0], [], {}, []
    while stack:
        sizes.append(len(stack))
        leaves, stops, grow = [], [], []
        for v in stack:
            if use_frustum and not any(SR.frustum_visible(xyz[v], F(bounds[v]), pl) for pl in pls):
                states[v] = 0
            elif nodes[v, CC] == 0:
                states[v] = 1
                leaves.append(v)
            elif use_lod and not SR.lod_expand(xyz[v], F(md2[v]), cam, dmul):
                states[v] = 2
                stops.append(v)
            else:
                states[v] = 3
                grow.append(v)
        cut += leaves + stops
        stack = next_frontier(nodes, grow)
    return np.array(cut, np.int32), states, sizes


def order_nary(nodes, max_entries=65535, max_levels=64):
    """F* (every node with children expands), the level starts (the last = M), and per F* entry the preorder position
    and end (position + subtree size) of the n-ary tree; None when the tree exceeds the flat cut's limits."""
    nodes = np.asarray(nodes)
    fs, lev, level = [], [], [0]
    while level:
        lev.append(len(fs))
        fs += level
        level = next_frontier(nodes, [v for v in level if nodes[v, CC] > 0])
    M = len(fs)
    if M > max_entries or len(lev) > max_levels:
        return None
    pos, end = {}, {}

    def visit(v, p):  # iterative preorder
        stack = [(v, 0)]
        pos[v] = p
        p += 1
        while stack:
            u, r = stack.pop()
            kids = children(nodes, u) if nodes[u, CC] > 0 else []
            if r < len(kids):
                stack.append((u, r + 1))
                pos[kids[r]] = p
                p += 1
                stack.append((kids[r], 0))
            else:
                end[u] = p
    visit(0, 0)
    return dict(nodes=np.array(fs, np.int32), level_starts=np.array(lev + [M], np.int32),
                pos=np.array([pos[v] for v in fs], np.int32), end=np.array([end[v] for v in fs], np.int32))
