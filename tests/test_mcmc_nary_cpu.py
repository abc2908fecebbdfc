"""The host side of the n-ary MCMC relocation (hlgs_core.mcmc.apply_relocation_nary, no GPU) against the sequential
model of tests/mcmc_nary_ref.py: the hand-derived 13-row tree of tests/spt_nary_cases.py, a tree in which a promoted
survivor is the parent of an unlink group, binary hierarchies (where the n-ary writes must leave the state of
apply_relocation), and the spawn on a merged scene.  The model's own selection is pinned on the hand tree and, on
binary hierarchies, against select_relocation."""
import numpy as np
import pytest
import torch

import mcmc_nary_ref as NR
import mcmc_ref as R
import spt_nary_cases as C
from hlgs_core import mcmc
from hlgs_core import synthetic as S

# dead rows -> the kept groups (parent, survivor, freed rows) on the hand tree
#        0
#      / | \
#     1  2  3          1 -> 4 -> (10, 11);  2 -> (5, 6, 7, 8, 9);  3 -> 12
HAND_CASES = [
    ((10,), [(4, 11, (10, 11))]),
    ((10, 11), [(4, 11, (10, 11))]),
    ((12,), []),                              # an only child is never relocated
    ((5,), []),                               # a single dead child of five waits
    ((6, 8), [(2, -1, (6, 8))]),
    ((5, 6, 7, 8), [(2, 9, (5, 6, 7, 8, 9))]),
    ((5, 6, 7, 8, 9), [(2, 9, (5, 6, 7, 8, 9))]),
    ((6, 8, 10), [(2, -1, (6, 8)), (4, 11, (10, 11))]),
]


def _equal_state(a, b):
    assert torch.equal(a[0], b[0])
    for k in R.NAMES:
        assert torch.equal(a[1][k], b[1][k]), k
        for m in ("exp_avgs", "exp_avgs_sqs"):
            assert torch.equal(a[2][k][m], b[2][k][m]), (k, m)


def _mask(size, dead):
    m = torch.zeros(size, dtype=torch.bool)
    m[list(dead)] = True
    return m


def _apply_both(nodes, storage, opt, sel, sky, size, rng, n=None):
    """apply_relocation_nary and the model on clones of one state, the first n groups (all of them by default) placed
    at the first alive rows; the lists are passed whole, and both sides cut them to the places."""
    gp, gs, st, fr, alive = sel
    n = len(gp) if n is None else n
    assert len(alive) >= n
    re = torch.tensor(alive[:n], dtype=torch.int64)
    new_op = torch.tensor(rng.normal(size=(n, 1)).astype(np.float32))
    new_sc = torch.tensor(rng.normal(size=(n, 3)).astype(np.float32))
    ref = R.clone_state(nodes, storage, opt)
    t = lambda a: torch.tensor(a, dtype=torch.int32)  # noqa: E731
    mcmc.apply_relocation_nary(nodes, storage, opt, t(gp), t(gs), t(st), t(fr), re, new_op, new_sc, sky, size)
    NR.relocation_nary_ref(ref[0], ref[1], ref[2], gp, gs, st, fr, re, new_op, new_sc, sky, size)
    _equal_state((nodes, storage, opt), ref)
    NR.check_links_nary(nodes, sky, size)
    return re


@pytest.mark.parametrize("dead,want", HAND_CASES)
def test_hand_tree(dead, want):
    rng = np.random.default_rng(len(dead))
    nodes, storage, opt = NR.make_nary_state(C.hand()[0], 16, rng)
    NR.check_links_nary(nodes, 0, 13)
    before = R.clone_state(nodes, storage, opt)
    sel = NR.select_nary_ref(nodes, _mask(13, dead), 13, 0)
    gp, gs, st, fr, alive = sel
    assert [(p, s, tuple(fr[a:b])) for p, s, a, b in zip(gp, gs, st, st[1:])] == want
    leaves = [5, 6, 7, 8, 9, 10, 11, 12]
    promoted = {s for _, s, _ in want}
    assert alive == [v for v in leaves if v not in dead and v not in promoted]
    re = _apply_both(nodes, storage, opt, sel, 0, 13, rng)
    assert not nodes[13:].any()
    if not want:
        _equal_state((nodes, storage, opt), before)
        return
    leaves_before = R.leaf_count(before[0], 0, 13)
    # a promote group turns its place into a parent and its parent's row into the survivor; an unlink group only the
    # first: leaves change by -1 per unlink group whose place was a leaf (it always is)
    assert R.leaf_count(nodes, 0, 13) == leaves_before - sum(1 for _, s, _ in want if s < 0)
    for g, (p, s, freed) in enumerate(want):
        r = int(re[g])
        assert NR.children(nodes, r) == list(freed)
        assert all(int(nodes[v, R.DEPTH]) == int(nodes[r, R.DEPTH]) + 1 for v in freed)
    if dead == (6, 8):
        assert NR.children(nodes, 2) == [5, 7, 9]
    if dead == (10,):
        # 11 moved into 4: row 4 is a leaf holding 11's parameters, and row 11 is a copy of 10 but for f_rest, rotation
        assert int(nodes[4, R.CHILD_COUNT]) == 0 and torch.equal(storage["xyz"][4], before[1]["xyz"][11])
        assert torch.equal(storage["xyz"][11], storage["xyz"][10])
        assert torch.equal(storage["f_rest"][11], before[1]["f_rest"][11])
        assert not opt["xyz"]["exp_avgs"][11].any() and opt["xyz"]["exp_avgs"][10].any()
    if len(dead) >= 4:
        # 9 moved into 2, which is now a leaf under the root
        assert int(nodes[2, R.CHILD_COUNT]) == 0 and torch.equal(storage["scaling"][2], before[1]["scaling"][9])


def test_promoted_survivor_is_an_unlink_parent():
    """0 -> (1, 2), 2 -> (3, 4, 5, 6); 1, 3 and 5 are dead: 2 is promoted into the root and, before that, loses two
    of its children, so 4 and 6 end as the children of the root."""
    rows = [[0, -1, 2, 1, 0, 70], [1, 0, 0, 2, 2, 71], [1, 0, 4, 3, 0, 72], [2, 2, 0, 4, 4, 73], [2, 2, 0, 5, 5, 74],
            [2, 2, 0, 6, 6, 75], [2, 2, 0, 7, 0, 76]]
    rng = np.random.default_rng(3)
    nodes, storage, opt = NR.make_nary_state(np.array(rows, np.int32), 8, rng)
    before = R.clone_state(nodes, storage, opt)
    sel = NR.select_nary_ref(nodes, _mask(7, (1, 3, 5)), 7, 0)
    assert sel == ([0, 2], [2, -1], [0, 2, 4], [1, 2, 3, 5], [4, 6])
    _apply_both(nodes, storage, opt, sel, 0, 7, rng)
    assert NR.children(nodes, 0) == [4, 6]
    assert nodes[4].tolist()[:3] == [1, 0, 2] and nodes[6].tolist()[:3] == [1, 0, 2]
    assert NR.children(nodes, 4) == [1, 2] and NR.children(nodes, 6) == [3, 5]
    assert nodes[:, 5].tolist() == [70, 71, 72, 73, 74, 75, 76, 0]
    for k in R.NAMES:  # the root holds what row 2 held
        assert torch.equal(storage[k][0], before[1][k][2]), k


@pytest.mark.parametrize("seed", range(6))
def test_binary_hierarchy_gives_the_binary_round(seed):
    """On a binary table built as tests/test_mcmc_cpu.py builds them: the model's selection is select_relocation's,
    and apply_relocation_nary leaves the state apply_relocation leaves."""
    rng = np.random.default_rng(2000 + seed)
    sky = 4
    leaves = int(rng.integers(64, 513))
    h = S.make_dynamic_hierarchy(S.make_gaussians(leaves, 0, S.make_camera(64, 48), seed=seed), skybox_points=sky,
                                 seed=seed)
    size = h["nodes"].shape[0]
    nodes, storage, opt = NR.make_nary_state(h["nodes"], size + 2 * leaves, rng)
    leaf_ids = torch.where(nodes[:size, R.CHILD_COUNT] == 0)[0]
    add = leaf_ids[torch.tensor(np.sort(rng.choice(leaves, size=leaves // 20 + 1, replace=False)))]
    rows = tuple(torch.tensor(rng.normal(size=(len(add),) + tuple(storage[k].shape[1:])).astype(np.float32))
                 for k in ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation"))
    new_size = mcmc.apply_spawn(nodes, storage, add, rows, size)
    NR.check_links_nary(nodes, sky, new_size)
    old_leaves = torch.where(nodes[:size, R.CHILD_COUNT] == 0)[0].numpy()
    dead_mask = torch.zeros(new_size, dtype=torch.bool)
    dead_mask[torch.tensor(rng.choice(old_leaves, size=max(2, len(old_leaves) // 10), replace=False))] = True
    pairs = [int(i) for i in old_leaves if nodes[i, R.NEXT_SIBLING] > 0
             and nodes[int(nodes[i, R.NEXT_SIBLING]), R.CHILD_COUNT] == 0][:3]
    for i in pairs:
        dead_mask[i] = dead_mask[int(nodes[i, R.NEXT_SIBLING])] = True
    dead, sib, alive = mcmc.select_relocation(nodes, dead_mask, new_size)
    n = len(dead)
    gp, gs, st, fr, al = NR.select_nary_ref(nodes, dead_mask, new_size, sky)
    assert gp == nodes[dead, R.PARENT].tolist() and gs == sib.tolist() and al == alive.tolist()
    assert st == list(range(0, 2 * n + 1, 2)) and fr == torch.stack([dead, sib.long()], 1).reshape(-1).tolist()
    assert NR.relocated_count(gs, st, n) == n
    reinit = alive[torch.tensor(rng.choice(len(alive), size=n, replace=False))]
    new_op = torch.tensor(rng.normal(size=(n, 1)).astype(np.float32))
    new_sc = torch.tensor(rng.normal(size=(n, 3)).astype(np.float32))
    ref = R.clone_state(nodes, storage, opt)
    model = R.clone_state(nodes, storage, opt)
    t = lambda a: torch.tensor(a, dtype=torch.int32)  # noqa: E731
    mcmc.apply_relocation_nary(nodes, storage, opt, t(gp), t(gs), t(st), t(fr), reinit, new_op, new_sc, sky, new_size)
    mcmc.apply_relocation(ref[0], ref[1], ref[2], dead, sib, reinit, new_op, new_sc, sky, new_size)
    _equal_state((nodes, storage, opt), ref)
    NR.relocation_nary_ref(model[0], model[1], model[2], gp, gs, st, fr, reinit, new_op, new_sc, sky, new_size)
    _equal_state((nodes, storage, opt), model)
    R.check_links(nodes, sky, new_size)
    NR.check_links_nary(nodes, sky, new_size)


@pytest.mark.parametrize("name,sky", [("k3", 0), ("wide", 0), ("chain", 0), ("k3", 4)])
def test_merged_scene_matches_the_model(name, sky):
    """Seeded flags on a fifth of the leaves of a merged scene: promote and unlink groups, lists of one, wide lists;
    fewer places than groups (the truncation of relocate_gs) in the k3 case with skybox rows."""
    nd = C.scene(name, sky)[0]
    size = nd.shape[0]
    rng = np.random.default_rng(7)
    nodes, storage, opt = NR.make_nary_state(nd, size, rng)
    NR.check_links_nary(nodes, sky, size)
    sel = NR.select_nary_ref(nodes, NR.seeded_flags(nd, sky), size, sky)
    gp, gs, st, fr, alive = sel
    assert len(gp) >= 2
    if name == "k3":
        assert any(s < 0 for s in gs) and any(s >= 0 for s in gs)
    if name == "wide":  # lists of up to 40 leaves: unlink groups of many rows
        assert max(b - a for a, b in zip(st, st[1:])) >= 5 and all(s < 0 for s in gs)
    _apply_both(nodes, storage, opt, sel, sky, size, rng, n=len(gp) // 2 if sky else None)


def test_k8_flags_cross_a_scan_block():
    """The GPU test's dense k8 case must put more than one scan block (2,048) of groups and of alive rows behind the
    scans; the model says so here, without a GPU.  A fifth of k8's 9,259 leaves is 1,851 flags, which cannot make
    2,048 groups, so that case flags NR.DENSE_SHARE of them."""
    nd = C.scene("k8")[0]
    gp, _, _, _, alive = NR.select_nary_ref(nd, NR.seeded_flags(nd, 0), nd.shape[0], 0)
    assert len(gp) == 1588 and len(alive) == 6043
    gp, _, _, _, alive = NR.select_nary_ref(nd, NR.seeded_flags(nd, 0, share=NR.DENSE_SHARE), nd.shape[0], 0)
    assert len(gp) > 2048 and len(alive) > 2048


def test_spawn_keeps_a_merged_scene():
    """apply_spawn needs no n-ary form: it reads child_count == 0, overwrites first_child and appends pairs."""
    nd = C.scene("k3")[0]
    size = nd.shape[0]
    rng = np.random.default_rng(11)
    leaf_ids = np.where(nd[:, R.CHILD_COUNT] == 0)[0]
    add = torch.tensor(np.sort(rng.choice(leaf_ids, size=len(leaf_ids) // 20, replace=False)))
    nodes, storage, opt = NR.make_nary_state(nd, size + 2 * len(add), rng)
    rows = tuple(torch.tensor(rng.normal(size=(len(add),) + tuple(storage[k].shape[1:])).astype(np.float32))
                 for k in ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation"))
    ref = R.clone_state(nodes, storage, opt)
    new_size = mcmc.apply_spawn(nodes, storage, add, rows, size)
    assert R.spawn_ref(ref[0], ref[1], add, rows, size) == new_size == size + 2 * len(add)
    _equal_state((nodes, storage, opt), ref)
    NR.check_links_nary(nodes, 0, new_size)
    assert R.leaf_count(nodes, 0, new_size) == len(leaf_ids) + len(add)
    # the untouched rows keep every column, the merger's first_child = id + 1 of the leaves included
    rest = np.setdiff1d(np.arange(size), add.numpy())
    assert torch.equal(nodes[rest], torch.tensor(nd)[rest])
