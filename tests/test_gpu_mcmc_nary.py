"""The MCMC densification round on an n-ary hierarchy on the GPU (csrc/mcmc_nary.hip, hlgs_core.mcmc.*_nary): the
device selection against the sequential model of tests/mcmc_nary_ref.py, every integer; relocate_gs_nary against
relocate_gs on a binary scene, bit for bit; and densify_round_nary around an SPTCache over a merged scene against the
model's round."""
import math

import numpy as np
import pytest
import torch

import mcmc_nary_ref as NR
import mcmc_ref as R
import spt_nary_cases as C
from hlgs_core import mcmc, spt

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _select(nd, mask, sky, size=None):
    size = nd.shape[0] if size is None else size
    out = mcmc.select_relocation_nary(torch.as_tensor(nd), mask, size, sky, DEV)
    assert all(t.is_cuda and t.dtype == torch.int32 for t in out)
    return tuple(t.cpu().tolist() for t in out)


def _assert_selection(nd, mask, sky):
    got = _select(nd, mask, sky)
    want = NR.select_nary_ref(nd, mask, nd.shape[0], sky)
    for name, g, w in zip(("group_parent", "group_survivor", "group_start", "free_rows", "alive"), got, want):
        assert g == w, name
    return got


# ------------------------------------------------------------------------------------------------ the selection
@pytest.mark.parametrize("dead", [(10,), (10, 11), (12,), (5,), (6, 8), (5, 6, 7, 8), (5, 6, 7, 8, 9), (6, 8, 10)])
def test_selection_on_the_hand_tree(dead):
    nd = C.hand()[0]
    mask = torch.zeros(13, dtype=torch.bool)
    mask[list(dead)] = True
    gp, gs, st, fr, _ = _assert_selection(nd, mask, 0)
    if dead == (6, 8, 10):
        assert (gp, gs, st, fr) == ([2, 4], [-1, 11], [0, 2, 4], [6, 8, 10, 11])


@pytest.mark.parametrize("name,sky", [("k3", 0), ("wide", 0), ("chain", 0), ("k3", 4), ("k8", 0)])
def test_selection_on_merged_scenes(name, sky):
    nd = C.scene(name, sky)[0]
    gp = _assert_selection(nd, NR.seeded_flags(nd, sky), sky)[0]
    assert len(gp) >= 2


def test_selection_larger_than_a_scan_block():
    """More than 2,048 (kScanItems) kept groups and alive rows: the group, offset and alive scans all cross a block."""
    nd = C.scene("k8")[0]
    gp, _, _, fr, alive = _assert_selection(nd, NR.seeded_flags(nd, 0, share=NR.DENSE_SHARE), 0)
    assert len(gp) > 2048 and len(alive) > 2048 and len(fr) > 2 * 2048


def test_flags_on_inner_rows_skybox_rows_and_the_root_are_ignored():
    sky = 4
    nd = C.scene("k3", sky)[0]
    leaves_only = NR.seeded_flags(nd, sky)
    mask = leaves_only.clone()
    mask[:sky + 1] = True                                     # the skybox rows and the root
    mask[torch.tensor(nd[:, R.CHILD_COUNT] > 0)] = True       # every inner row
    assert _assert_selection(nd, mask, sky) == _select(nd, leaves_only, sky)


def test_nothing_to_select_launches_nothing():
    empty = ([], [], [0], [], [])
    assert _select(np.zeros((0, 6), np.int32), torch.zeros(0, dtype=torch.bool), 0) == empty
    # an all-clear mask returns before the table is read: a malformed one raises nothing
    bad = C.malformed()["member_out_of_range"]
    assert _select(bad, torch.zeros(13, dtype=torch.bool), 0) == empty
    assert _select(C.hand()[0], torch.ones(13, dtype=torch.bool), 0, size=0) == empty
    # flags that select nothing still list the respawn candidates
    mask = torch.zeros(13, dtype=torch.bool)
    mask[5] = True
    assert _select(C.hand()[0], mask, 0) == ([], [], [0], [], [6, 7, 8, 9, 10, 11, 12])


@pytest.mark.parametrize("name", sorted(C.malformed()))
def test_malformed_table_is_rejected_and_the_next_selection_is_right(name):
    mask = torch.zeros(13, dtype=torch.bool)
    mask[[6, 8, 10]] = True
    with pytest.raises(RuntimeError, match="n-ary contract"):
        _select(C.malformed()[name], mask, 0)
    _assert_selection(C.hand()[0], mask, 0)


# ------------------------------------------------------------------------------------------------ binary equivalence
def _moments(storage, seed):
    g = torch.Generator().manual_seed(seed)
    return {k: {m: torch.randn(v.shape, generator=g) for m in ("exp_avgs", "exp_avgs_sqs")}
            for k, v in storage.items()}


def _equal_state(a, b):
    assert torch.equal(a[0], b[0])
    for k in R.NAMES:
        assert torch.equal(a[1][k], b[1][k]), k
        for m in ("exp_avgs", "exp_avgs_sqs"):
            assert torch.equal(a[2][k][m], b[2][k][m]), (k, m)


def test_relocate_gs_nary_equals_relocate_gs_on_a_binary_scene():
    import test_gpu_mcmc as TM
    nodes, storage, _, size, low = TM._scene()
    opt = _moments(storage, 3)
    mask = torch.zeros(size, dtype=torch.bool)
    mask[low] = True
    pairs = [int(i) for i in torch.where(nodes[:size, R.CHILD_COUNT] == 0)[0] if nodes[i, R.NEXT_SIBLING] > 0
             and nodes[int(nodes[i, R.NEXT_SIBLING]), R.CHILD_COUNT] == 0][:5]
    for i in pairs:  # whole sibling pairs among the dead: one of each stays
        mask[i] = mask[int(nodes[i, R.NEXT_SIBLING])] = True
    ref = R.clone_state(nodes, storage, opt)
    want = mcmc.relocate_gs(ref[1], ref[2], ref[0], mask, size, TM.SKY, seed=11)
    got = mcmc.relocate_gs_nary(storage, opt, nodes, mask, size, TM.SKY, seed=11)
    assert got == want and want >= len(low) // 2
    _equal_state((nodes, storage, opt), ref)
    R.check_links(nodes, TM.SKY, size)


# ------------------------------------------------------------------------------------------------ the round
SPT_ARGS = dict(SPT_Root_Volume=2.5e-5, target_granularity=C.TG, min_SPT_Size=10)
SHAPES = {"xyz": (3,), "f_dc": (1, 3), "opacity": (1,), "scaling": (3,), "rotation": (4,), "f_rest": (15, 3)}
_merged = {}


def _merged_scene():
    """The merged k3 scene as a training state with spare capacity (1.3x its rows): its own positions and scales,
    random other parameters and moments, a tenth of the leaves at opacity 0.001.  Built once; the tests clone it."""
    if not _merged:
        nd, xyz, scaling = C.tensors("k3")
        G = nd.shape[0]
        cap = int(1.3 * G)
        rng = np.random.default_rng(21)
        nodes = torch.zeros((cap, 6), dtype=torch.int32)
        nodes[:G] = nd
        storage = {k: torch.zeros((cap,) + SHAPES[k]) for k in R.NAMES}
        for k in R.NAMES:
            storage[k][:G] = torch.tensor(rng.normal(size=(G,) + SHAPES[k]).astype(np.float32))
        storage["xyz"][:G], storage["scaling"][:G] = xyz, scaling
        leaves = torch.where(nd[:, R.CHILD_COUNT] == 0)[0]
        low = leaves[torch.tensor(rng.choice(len(leaves), size=len(leaves) // 10, replace=False))]
        storage["opacity"][low] = math.log(0.001 / 0.999)
        # and the first two leaves of every list of four or more that has them, so that the round unlinks as well
        for p in torch.where(nd[:, R.CHILD_COUNT] >= 4)[0].tolist():
            kids = [c for c in NR.children(nd, p) if nd[c, R.CHILD_COUNT] == 0][:2]
            if len(kids) == 2:
                storage["opacity"][kids] = math.log(0.001 / 0.999)
        opt = {k: {m: torch.zeros((cap,) + SHAPES[k]) for m in ("exp_avgs", "exp_avgs_sqs")} for k in R.NAMES}
        for k in R.NAMES:
            for m in ("exp_avgs", "exp_avgs_sqs"):
                opt[k][m][:G] = torch.tensor(rng.random(size=(G,) + SHAPES[k]).astype(np.float32))
        b = spt.build_hierarchical_spt(nd, xyz, scaling, 0, *SPT_ARGS.values(), nary=True)
        _merged.update(nodes=nodes, storage=storage, opt=opt, spt=b, size=G, low=low)
    m = _merged
    nodes, storage, opt = R.clone_state(m["nodes"], m["storage"], m["opt"])
    return nodes, storage, opt, m["spt"], m["size"], m["low"]


def _round(on_device, seed=5):
    import test_gpu_spt_nary as TN
    from hlgs_core.spt_cache import SPTCache
    nodes, storage, opt, b, size, low = _merged_scene()
    cache = SPTCache(storage, b, 0, opt_storage=opt)
    assert cache.nary
    cams = TN._ring_cameras([1.5, 1.5, 0.0], 1.0, n=7)
    cache.step(cams[0]["projmatrix"], cams[0]["campos"])
    new_size = mcmc.densify_round_nary(cache, nodes, size, cap_max=10 ** 9, seed=seed, spt_args=SPT_ARGS,
                                       spt_on_device=on_device)
    return cache, nodes, size, new_size, cams


def _model_round(seed):
    """The round on host copies, one node at a time, with the places the sampler draws for the same inputs."""
    nodes, storage, opt, _, size, _ = _merged_scene()
    threshold = mcmc._inverse_sigmoid(torch.tensor(0.005)).item()
    dead_indices = torch.where(storage["opacity"][:size, 0] <= threshold)[0]
    num = (min(10 ** 9, int(1.05 * size)) - size) // 2
    leaves = torch.where(nodes[:size, R.CHILD_COUNT] == 0)[0]
    _, counts = mcmc.sample_alive(storage["opacity"][:size].to(DEV), num, leaves, seed=seed,
                                  stream=mcmc.STREAM_SPAWN, size=size)
    add = torch.where(counts == 1)[0].cpu()
    rows = mcmc.update_params(storage, add, torch.ones((size,), dtype=torch.int32))
    new_size = R.spawn_ref(nodes, storage, add, [r.cpu() for r in rows], size)
    mask = torch.zeros(new_size, dtype=torch.bool)
    mask[dead_indices] = True
    mask &= nodes[:new_size, R.CHILD_COUNT] == 0
    gp, gs, st, fr, alive = NR.select_nary_ref(nodes, mask, new_size, 0)
    reinit, counts = mcmc.sample_alive(storage["opacity"][:new_size].to(DEV), 2 * len(gp),
                                       torch.tensor(alive), seed=seed, stream=mcmc.STREAM_RELOCATE, size=new_size)
    reinit = reinit.unique().cpu().long()
    g = torch.Generator()
    g.manual_seed(seed)
    reinit = reinit[torch.randperm(len(reinit), generator=g)[:len(gp)]]
    rows = mcmc.update_params(storage, reinit, counts)
    NR.relocation_nary_ref(nodes, storage, opt, gp, gs, st, fr, reinit, rows[3].cpu(), rows[4].cpu(), 0, new_size)
    return nodes, storage, opt, new_size, len(add), (gp, gs, st, len(reinit))


def test_densify_round_nary_on_a_merged_scene():
    cache, nodes, size, new_size, cams = _round(False)
    want = _model_round(5)
    n_add, (gp, gs, st, n_places) = want[4], want[5]
    assert new_size == want[3] == size + 2 * n_add and 0 < new_size - size <= int(1.05 * size) - size
    assert len(gp) >= 20 and any(s < 0 for s in gs) and any(s >= 0 for s in gs) and n_places >= 20
    NR.check_links_nary(nodes, 0, new_size)
    assert not nodes[new_size:].any()
    _equal_state((nodes, cache.storage, cache.opt_storage), want[:3])
    # the cache streams the rebuilt SPTs
    assert cache.nary and cache.render_indices.numel() == 0
    cache.step(cams[1]["projmatrix"], cams[1]["campos"])
    idx = cache.render_indices.cpu().long()
    # (row 1, the root of an SPT and a row of the upper cut, is resident twice on this scene before any round too)
    assert idx.numel() > 10 and int(idx.max()) < new_size and int(idx.min()) >= 0
    cache.sync_storage()
    for k in R.NAMES:
        assert torch.equal(cache.params[k].detach().cpu(), cache.storage[k][idx]), k
    # the binary round still refuses this cache, and leaves it alone
    before = cache.host.clone()
    with pytest.raises(ValueError, match="binary"):
        mcmc.densify_round(cache, nodes, new_size, cap_max=10 ** 9, seed=5, spt_args=SPT_ARGS)
    torch.cuda.synchronize()
    assert torch.equal(cache.host, before)


def test_densify_round_nary_with_the_device_spt_build_is_identical():
    host = _round(False)
    dev = _round(True)
    assert host[3] == dev[3] and torch.equal(host[1], dev[1]) and torch.equal(host[0].host, dev[0].host)
    cam = host[4][2]
    a = host[0].step(cam["projmatrix"], cam["campos"])
    b = dev[0].step(cam["projmatrix"], cam["campos"])
    assert a.numel() > 0 and torch.equal(a, b)


def test_densify_round_nary_on_a_binary_cache_equals_densify_round():
    import test_gpu_mcmc as TM
    from hlgs_core.spt_cache import SPTCache
    out = []
    for fn in (mcmc.densify_round, mcmc.densify_round_nary):
        nodes, storage, b, size, _ = TM._scene()
        cache = SPTCache(storage, b, TM.SKY)
        cam = TM._cams()[0]
        cache.step(cam["projmatrix"], cam["campos"])
        out.append((fn(cache, nodes, size, cap_max=10 ** 9, seed=11, spt_args=TM.SPT_ARGS), nodes, cache))
    assert out[0][0] == out[1][0] and torch.equal(out[0][1], out[1][1]) and torch.equal(out[0][2].host, out[1][2].host)
    assert not out[1][2].nary
    for k in ("spt_starts", "spt_gidx", "nodes"):
        assert torch.equal(getattr(out[0][2], k), getattr(out[1][2], k)), k
