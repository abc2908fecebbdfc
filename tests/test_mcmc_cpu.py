"""The host side of the MCMC densification round (hlgs_core/mcmc.py, csrc/hlgs_rng.h): Philox known answers, the
uniform mapping of hlgs_rng_uniform_host, and the hierarchy writes of add_new_gs / relocate_gs (apply_spawn,
select_relocation, apply_relocation -- the sample is passed in, so no GPU) against a hand-written node table, against
the loop-per-node restatement of tests/mcmc_ref.py on random hierarchies, and against the link invariants."""
import numpy as np
import pytest
import torch

import mcmc_ref as R
from hlgs_core import mcmc
from hlgs_core import synthetic as S


@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, want):
    assert " ".join(f"{w:08x}" for w in R.philox4x32_10(counter, key)) == want


@pytest.mark.parametrize("seed,stream,first,n", [(0, 0, 0, 5), (0xFFFFFFFFFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFFFFFFFFF0, 8),
                                                 (0x299F31D0A4093822, 0x13198A2E, 0x85A308D3243F6A88, 1),
                                                 (12345, 7, (1 << 32) - 3, 7)])
def test_uniform_host_equals_python_mapping(seed, stream, first, n):
    """hlgs_rng_uniform_host runs the library's own Philox (csrc/hlgs_rng.h): its numbers are the pure-Python Philox's
    words mapped to 53 bits, exactly -- the first case's first number comes from the counter-0 / key-0 known answer,
    the second and third from the all-ones and the pi-digits ones."""
    got = mcmc.rng_uniform_host(seed, stream, first, n).numpy()
    want = R.uniforms(seed, stream, first, n)
    np.testing.assert_array_equal(got, want)
    assert (got >= 0).all() and (got < 1).all()
    if seed == 0:
        assert got[0] == ((0x6627E8D5 >> 5) * 2.0 ** 26 + (0xE169C58D >> 6)) * 2.0 ** -53


def _tiny_tree():
    """Two skybox rows and nine nodes (the seven-node tree has a single respawn candidate once two leaves are dead
    and one leaf is a sibling; this one has two):
        2 -+- 3 (leaf, dead; its sibling 4 is an interior node)
           +- 4 -+- 5 -+- 6 (leaf, dead; its sibling 7 is a leaf)
                 |     +- 7
                 +- 8 -+- 9
                       +- 10"""
    rows = [[-99] * 6, [-99] * 6, [0, -1, 2, 3, 0, 20], [1, 2, 0, 0, 4, 30], [1, 2, 2, 5, 0, 40], [2, 4, 2, 6, 8, 50],
            [3, 5, 0, 0, 7, 60], [3, 5, 0, 0, 0, 70], [2, 4, 2, 9, 0, 80], [3, 8, 0, 0, 10, 90], [3, 8, 0, 0, 0, 100]]
    cap = 16
    nodes = torch.zeros((cap, 6), dtype=torch.int32)
    nodes[:11] = torch.tensor(rows, dtype=torch.int32)
    marker = torch.arange(cap, dtype=torch.float32)
    storage = {k: marker.reshape((cap,) + (1,) * len(R.SHAPES[k])).expand((cap,) + R.SHAPES[k]).clone()
               for k in R.NAMES}
    opt = {k: {m: torch.ones((cap,) + R.SHAPES[k]) for m in ("exp_avgs", "exp_avgs_sqs")} for k in R.NAMES}
    return nodes, storage, opt


def _markers(t, n):
    return t[:n].reshape(n, -1)[:, 0].tolist()


def test_relocation_hand_written_tree():
    nodes, storage, opt = _tiny_tree()
    dead_mask = torch.zeros(11, dtype=torch.bool)
    dead_mask[[3, 6]] = True
    dead, sib, alive = mcmc.select_relocation(nodes, dead_mask, 11)
    assert dead.tolist() == [3, 6] and sib.tolist() == [4, 7] and alive.tolist() == [9, 10]
    new_op = torch.tensor([[103.0], [106.0]])
    new_sc = torch.tensor([[203.0] * 3, [206.0] * 3])
    mcmc.apply_relocation(nodes, storage, opt, dead, sib, torch.tensor([9, 10]), new_op, new_sc, 2, 11)
    want = [[-99] * 6, [-99] * 6,
            [0, -1, 2, 5, 0, 20],    # the root took the children of the promoted 4
            [4, 9, 0, 0, 4, 30],     # dead 3: first child of 9
            [4, 9, 0, 0, 0, 40],     # its former sibling 4: second child of 9, now a leaf
            [1, 2, 0, 0, 8, 50],     # 5 took the leaf 7's place: a leaf, one level up with its sibling 8
            [4, 10, 0, 0, 7, 60],    # dead 6: first child of 10
            [4, 10, 0, 0, 0, 70],
            [1, 2, 2, 9, 0, 80],
            [3, 8, 2, 3, 10, 90],    # 9 and 10 keep their (now stale) depth 3
            [3, 8, 2, 6, 0, 100]]
    assert nodes[:11].tolist() == want
    assert not nodes[11:].any()
    assert _markers(storage["xyz"], 11) == [0, 1, 4, 9, 9, 7, 10, 10, 8, 9, 10]
    assert _markers(storage["f_dc"], 11) == [0, 1, 4, 9, 9, 7, 10, 10, 8, 9, 10]
    assert _markers(storage["opacity"], 11) == [0, 1, 4, 103, 103, 7, 106, 106, 8, 9, 10]
    assert _markers(storage["scaling"], 11) == [0, 1, 4, 203, 203, 7, 206, 206, 8, 9, 10]
    # the sibling copy leaves f_rest and rotation out (:1684-1689)
    assert _markers(storage["f_rest"], 11) == [0, 1, 4, 9, 4, 7, 10, 7, 8, 9, 10]
    assert _markers(storage["rotation"], 11) == [0, 1, 4, 9, 4, 7, 10, 7, 8, 9, 10]
    for k in R.NAMES:
        for m in ("exp_avgs", "exp_avgs_sqs"):
            assert _markers(opt[k][m], 11) == [1, 1, 1, 1, 0, 1, 1, 0, 1, 1, 1]
    R.check_links(nodes, 2, 11)
    assert R.leaf_count(nodes, 2, 11) == 5


def test_spawn_hand_written_tree():
    nodes, storage, _ = _tiny_tree()
    add = torch.tensor([7, 9])
    rows = tuple(torch.full((2,) + R.SHAPES[k], 300.0) + torch.tensor([7.0, 9.0]).reshape((2,) + (1,) * len(R.SHAPES[k]))
                 for k in ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation"))
    assert mcmc.apply_spawn(nodes, storage, add, rows, 11) == 15
    assert nodes[7].tolist() == [3, 5, 2, 11, 0, 70] and nodes[9].tolist() == [3, 8, 2, 13, 10, 90]
    assert nodes[11:16].tolist() == [[4, 7, 0, 0, 12, 0], [4, 7, 0, 0, 0, 0], [4, 9, 0, 0, 14, 0], [4, 9, 0, 0, 0, 0],
                                     [0] * 6]
    for k in R.NAMES:
        assert _markers(storage[k], 16) == list(range(11)) + [307, 307, 309, 309, 15]
    R.check_links(nodes, 2, 15)
    assert R.leaf_count(nodes, 2, 15) == 7
    with pytest.raises(RuntimeError, match="capacity"):
        mcmc.apply_spawn(nodes, storage, torch.tensor([11]), tuple(r[:1] for r in rows), 15)


def _equal_state(a, b):
    assert torch.equal(a[0], b[0])
    for k in R.NAMES:
        assert torch.equal(a[1][k], b[1][k]), k
        for m in ("exp_avgs", "exp_avgs_sqs"):
            assert torch.equal(a[2][k][m], b[2][k][m]), (k, m)


@pytest.mark.parametrize("seed", range(20))
def test_spawn_and_relocation_match_restatement(seed):
    rng = np.random.default_rng(1000 + seed)
    sky = 4
    leaves = int(rng.integers(64, 513))
    h = S.make_dynamic_hierarchy(S.make_gaussians(leaves, 0, S.make_camera(64, 48), seed=seed), skybox_points=sky,
                                 seed=seed)
    size = h["nodes"].shape[0]
    cap = size + 2 * leaves
    nodes = torch.zeros((cap, 6), dtype=torch.int32)
    nodes[:size] = torch.tensor(h["nodes"])
    storage, opt = R.make_storage(cap, rng)
    R.check_links(nodes, sky, size)
    n_leaves = R.leaf_count(nodes, sky, size)
    assert n_leaves == leaves
    # spawn at a random subset of the leaves
    leaf_ids = torch.where(nodes[:size, R.CHILD_COUNT] == 0)[0]
    add = leaf_ids[torch.tensor(np.sort(rng.choice(leaves, size=leaves // 20 + 1, replace=False)))]
    rows = tuple(torch.tensor(rng.normal(size=(len(add),) + R.SHAPES[k]).astype(np.float32))
                 for k in ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation"))
    ref = R.clone_state(nodes, storage, opt)
    new_size = mcmc.apply_spawn(nodes, storage, add, rows, size)
    assert R.spawn_ref(ref[0], ref[1], add, rows, size) == new_size == size + 2 * len(add)
    _equal_state((nodes, storage, opt), ref)
    R.check_links(nodes, sky, new_size)
    # dead leaves among those that existed before the spawn, with whole sibling pairs among them
    old_leaves = torch.where(nodes[:size, R.CHILD_COUNT] == 0)[0].numpy()
    dead_mask = torch.zeros(new_size, dtype=torch.bool)
    dead_mask[torch.tensor(rng.choice(old_leaves, size=max(2, len(old_leaves) // 10), replace=False))] = True
    pairs = [int(i) for i in old_leaves if nodes[i, R.NEXT_SIBLING] > 0
             and nodes[int(nodes[i, R.NEXT_SIBLING]), R.CHILD_COUNT] == 0][:3]
    for i in pairs:
        dead_mask[i] = dead_mask[int(nodes[i, R.NEXT_SIBLING])] = True
    dead, sib, alive = mcmc.select_relocation(nodes, dead_mask, new_size)
    d2, s2, a2 = R.select_ref(nodes, dead_mask, new_size)
    assert dead.tolist() == d2 and sib.tolist() == s2 and alive.tolist() == a2
    assert len(pairs) > 0 and all(int(nodes[i, R.NEXT_SIBLING]) not in d2 for i in pairs)
    reinit = alive[torch.tensor(rng.choice(len(alive), size=len(dead), replace=False))]
    new_op = torch.tensor(rng.normal(size=(len(dead), 1)).astype(np.float32))
    new_sc = torch.tensor(rng.normal(size=(len(dead), 3)).astype(np.float32))
    ref = R.clone_state(nodes, storage, opt)
    mcmc.apply_relocation(nodes, storage, opt, dead, sib, reinit, new_op, new_sc, sky, new_size)
    R.relocation_ref(ref[0], ref[1], ref[2], dead, sib, reinit, new_op, new_sc, sky, new_size)
    _equal_state((nodes, storage, opt), ref)
    R.check_links(nodes, sky, new_size)
    assert R.leaf_count(nodes, sky, new_size) == n_leaves + len(add)
    assert not nodes[new_size:].any()


def test_build_reports_no_variant_switches():
    from hlgs_core import build
    assert build.variant_switches() == []
    assert "mcmc.hip" in build.SOURCES
