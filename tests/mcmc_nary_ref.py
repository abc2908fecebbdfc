"""The n-ary relocation of the MCMC round as a plain sequential model, one node at a time, in the style of
tests/mcmc_ref.py: the specification that hlgs_core.mcmc.select_relocation_nary (csrc/mcmc_nary.hip) and
apply_relocation_nary are tested against (tests/test_mcmc_nary_cpu.py, tests/test_gpu_mcmc_nary.py).

The reference defines nothing here (relocate_gs, scene/gaussian_model.py:1588-1698, handles sibling pairs); the rules
are those of include/hlgs.h ("n-ary relocation") and DESIGN.md section 5b, chosen so that a binary hierarchy gives
the binary round.  For row v: P parent, C child_count, F first_child, N next_sibling (0 ends a list); the children of
p are C(p) rows: F(p), then the N links."""
import numpy as np
import torch

from mcmc_ref import CHILD_COUNT, DEPTH, FIRST_CHILD, NAMES, NEXT_SIBLING, PARENT


def children(nodes, p):
    out, c = [], int(nodes[p, FIRST_CHILD])
    for _ in range(int(nodes[p, CHILD_COUNT])):
        out.append(c)
        c = int(nodes[c, NEXT_SIBLING])
    return out


def select_nary_ref(nodes, dead_mask, size, sky):
    """The selection, per parent.  Returns (group_parent, group_survivor, group_start, free_rows, alive) as lists:
    the kept groups ascending by their first freed row, survivor -1 for an unlink group, group g's freed rows
    free_rows[group_start[g]:group_start[g + 1]]."""
    def candidate(v):
        return bool(dead_mask[v]) and v >= sky and int(nodes[v, CHILD_COUNT]) == 0 and int(nodes[v, PARENT]) >= 0
    groups = []
    for p in range(sky, size):
        kids = children(nodes, p)
        c = len(kids)
        if c == 0:
            continue
        dead = [v for v in kids if candidate(v)]
        if len(dead) == c:  # every child wants to die: the last one stays (:1597-1599)
            dead = dead[:-1]
        k = len(dead)
        a = c - k
        if k == 0:
            continue
        if a == 1:  # promote: the survivor moves into p and its row is freed behind the dead ones
            s = [v for v in kids if v not in dead][0]
            freed = dead + [s]
        else:       # unlink: p keeps its survivors
            s = -1
            freed = dead
        if len(freed) < 2:  # a single dead child of a wide list waits: a respawn place with one child deepens the tree
            continue
        groups.append((freed[0], p, s, freed))
    groups.sort()
    survivors = {g[2] for g in groups}
    alive = [v for v in range(sky, size) if int(nodes[v, CHILD_COUNT]) == 0 and not dead_mask[v]
             and v not in survivors]
    start, free = [0], []
    for _, _, _, freed in groups:
        free += freed
        start.append(len(free))
    return [g[1] for g in groups], [g[2] for g in groups], start, free, alive


def relocation_nary_ref(nodes, storage, opt, group_parent, group_survivor, group_start, free_rows, re, new_opacity,
                        new_scaling, sky, size):
    """The writes, per node, for the first len(re) groups; group g respawns at the leaf re[g]."""
    re = [int(v) for v in re]
    n = len(re)
    if n == 0:
        return
    gp, gs = [int(v) for v in group_parent[:n]], [int(v) for v in group_survivor[:n]]
    st = [int(v) for v in group_start[:n + 1]]
    freed = [[int(v) for v in free_rows[st[g]:st[g + 1]]] for g in range(n)]
    dead = [f[:-1] if gs[g] >= 0 else f for g, f in enumerate(freed)]
    # 1. every dead member takes the parameters of its group's place
    for g in range(n):
        for d in dead[g]:
            for name in ("xyz", "f_dc", "f_rest", "rotation"):
                storage[name][d] = storage[name][re[g]]
    for g in range(n):
        for d in dead[g]:
            storage["opacity"][d] = new_opacity[g]
            storage["scaling"][d] = new_scaling[g]
    # 2. unlink groups: the parent's list is rewritten to its survivors in their old order
    for g in range(n):
        if gs[g] >= 0:
            continue
        p = gp[g]
        keep = [v for v in children(nodes, p) if v not in dead[g]]
        nodes[p, FIRST_CHILD] = keep[0]
        for a, b in zip(keep, keep[1:] + [0]):
            nodes[a, NEXT_SIBLING] = b
        nodes[p, CHILD_COUNT] = len(keep)
    # 3. promote groups, deepest survivor first (:1641-1664)
    for depth in range(max(int(nodes[i, DEPTH]) for i in range(sky, size)), 0, -1):
        level = [g for g in range(n) if gs[g] >= 0 and int(nodes[gs[g], DEPTH]) == depth]
        for g in level:
            s, p = gs[g], gp[g]
            for name in NAMES:
                storage[name][p] = storage[name][s]
            nodes[p, CHILD_COUNT] = nodes[s, CHILD_COUNT]
            nodes[p, FIRST_CHILD] = nodes[s, FIRST_CHILD]
            for c in children(nodes, s):  # a leaf survivor has none (A-26); grandchildren keep their depth (A-29)
                nodes[c, PARENT] = p
                nodes[c, DEPTH] = int(nodes[p, DEPTH]) + 1
    # 4. the place becomes the parent of the freed rows, chained in order; column 5 is kept
    for g in range(n):
        nodes[re[g], CHILD_COUNT] = len(freed[g])
        nodes[re[g], FIRST_CHILD] = freed[g][0]
    for g in range(n):
        for v, nxt in zip(freed[g], freed[g][1:] + [0]):
            nodes[v] = torch.tensor([int(nodes[re[g], DEPTH]) + 1, re[g], 0, 0, nxt, int(nodes[v, 5])],
                                    dtype=torch.int32)
    # 5. a promoted survivor's row is a copy of the first freed row (A-25: not f_rest, not rotation), moments zeroed
    for g in range(n):
        if gs[g] < 0:
            continue
        for name in ("xyz", "opacity", "f_dc", "scaling"):
            storage[name][gs[g]] = storage[name][freed[g][0]]
    for g in range(n):
        if gs[g] < 0:
            continue
        for name in NAMES:
            opt[name]["exp_avgs"][gs[g]] = 0
            opt[name]["exp_avgs_sqs"][gs[g]] = 0


def relocated_count(group_survivor, group_start, n):
    """The dead Gaussians relocated by the first n groups: the sum of k."""
    return int(group_start[n]) - sum(1 for s in group_survivor[:n] if s >= 0)


def check_links_nary(nodes, sky, size, root=None):
    """The link invariants of an n-ary hierarchy over rows [sky, size): every list has child_count members inside
    (sky, size) and ends in next_sibling 0, every member's parent points back, and every row but the root is a member
    of exactly one list.  (Depth is not checked: a promoted node's grandchildren keep a stale depth, A-29.)"""
    nd = np.asarray(nodes[:size].cpu().numpy(), np.int64)
    root = sky if root is None else root
    seen = np.zeros(size, np.int64)
    assert (nd[sky:, CHILD_COUNT] >= 0).all()
    for p in range(sky, size):
        c, n = int(nd[p, FIRST_CHILD]), int(nd[p, CHILD_COUNT])
        for j in range(n):
            assert sky <= c < size and c != root, (p, j, c)
            assert nd[c, PARENT] == p, (p, c, nd[c, PARENT])
            seen[c] += 1
            last, c = c, int(nd[c, NEXT_SIBLING])
            assert (c == 0) == (j == n - 1), (p, j, last, c)
    want = np.ones(size, np.int64)
    want[:sky] = 0
    want[root] = 0
    np.testing.assert_array_equal(seen, want)
    assert nd[root, PARENT] == -1


DENSE_SHARE = 0.4  # of the k8 scene's leaves: 2,828 kept groups and 3,537 alive rows, both more than a scan block


def seeded_flags(nodes_np, sky, seed=0, share=0.2):
    """Dead flags (torch bool, one per row) on a seeded `share` of the leaves of rows [sky, size)."""
    leaves = np.where(nodes_np[sky:, CHILD_COUNT] == 0)[0] + sky
    rng = np.random.default_rng(seed)
    mask = torch.zeros(nodes_np.shape[0], dtype=torch.bool)
    mask[torch.tensor(rng.choice(leaves, size=int(share * len(leaves)), replace=False))] = True
    return mask


def make_nary_state(nodes_np, cap, rng, sh_rows=3):
    """(nodes, storage, opt): the node table padded to cap rows, random parameters and moments (mcmc_ref.make_storage
    shapes, f_rest with sh_rows rows)."""
    from mcmc_ref import SHAPES
    shapes = dict(SHAPES, f_rest=(sh_rows, 3))
    nodes = torch.zeros((cap, 6), dtype=torch.int32)
    nodes[:nodes_np.shape[0]] = torch.tensor(nodes_np)
    storage = {k: torch.tensor(rng.normal(size=(cap,) + shapes[k]).astype(np.float32)) for k in NAMES}
    opt = {k: {m: torch.tensor(rng.normal(size=(cap,) + shapes[k]).astype(np.float32))
               for m in ("exp_avgs", "exp_avgs_sqs")} for k in NAMES}
    return nodes, storage, opt
