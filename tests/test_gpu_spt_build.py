"""The SPT build on the GPU (csrc/spt_build.hip, hlgs_core.spt.build_hierarchical_spt_device) against the host build
(csrc/spt_build.cpp) on the same inputs, and against the reference's own run where a fixture holds one.

Every input first passes the check of tests/test_spt_build.py on the CPU: the host build and the torch restatement
(oracle/spt_ref.py) agree on every integer output, so no decision of that input sits within an exp rounding of a
tie.  Then SPT_starts, SPT_gaussian_indices, SPT_root_hierarchy_indices, upper_tree_nodes, upper_tree_xyz and
upper_tree_scaling are compared exactly, and SPT_max, SPT_min, min_distance_squared and bounding_sphere_radii at
rtol 2e-6 (the tolerance of tests/test_spt_build.py:30).  CPU references are computed once per input and shared."""
import os

import numpy as np
import pytest
import torch

from hlgs_core import mcmc, spt
from hlgs_core import synthetic as S
from oracle import spt_ref as SR

pytestmark = pytest.mark.gpu
DEV = "cuda"
EXACT = ("SPT_starts", "SPT_gaussian_indices", "SPT_root_hierarchy_indices", "upper_tree_nodes", "upper_tree_xyz",
         "upper_tree_scaling")
CLOSE = ("SPT_max", "SPT_min", "min_distance_squared", "bounding_sphere_radii")
INTS = ("SPT_starts", "SPT_gaussian_indices", "SPT_root_hierarchy_indices", "upper_tree_nodes")
TG = 0.02
GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "golden_spt.npz"))
GOLD_CASES = sorted({int(k.split("_")[-1]) for k in GOLD.files if k.startswith("params_")})


def _np(d):
    return {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else v) for k, v in d.items()}


def _restatement(*args):
    """oracle.spt_ref.build_spt.  Where the upper tree is the root alone, the restatement's one-node branch of
    get_min_distance returns a 0-dim tensor and its `md2[0] = ...` raises IndexError, after every integer output is
    final; only then it is run again with that result given its index's shape, which changes no value."""
    try:
        return SR.build_spt(*args)
    except IndexError:
        from unittest import mock
        plain = SR._min_distance
        with mock.patch.object(SR, "_min_distance", lambda n, s, idx, tg: plain(n, s, idx, tg).reshape(idx.shape)):
            ref = SR.build_spt(*args)
        assert ref["upper_tree_nodes"].shape[0] == 1
        return ref


def _host_reference(nodes, xyz, scaling, root, volume, tg, min_size):
    """The host build (with bounding spheres) of an input that passes the restatement check on its integer outputs."""
    want = spt.build_hierarchical_spt(nodes, xyz, scaling, root, volume, tg, min_size)
    ref = _restatement(nodes, xyz, scaling, root, volume, tg, min_size)
    for k in INTS:
        np.testing.assert_array_equal(want[k].numpy(), ref[k].numpy(), err_msg=f"host build against restatement: {k}")
    return _np(want)


def _compare(got, want, spheres=True):
    got = _np(got)
    assert set(got) == set(EXACT + CLOSE)
    for k in EXACT:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    for k in CLOSE:
        if k == "bounding_sphere_radii" and not spheres:
            assert got[k] is None
            continue
        assert got[k].shape == want[k].shape, k
        np.testing.assert_allclose(got[k], want[k], rtol=2e-6, atol=0, err_msg=k)


_inputs = {}


def _hierarchy(n, sky):
    """(nodes, xyz, log-scales) of the synthetic hierarchy of tests/test_spt_build.py."""
    if (n, sky) not in _inputs:
        h = S.make_dynamic_hierarchy(S.make_gaussians(n, 0, S.make_camera(256, 192), seed=n), skybox_points=sky,
                                     seed=n)
        nodes = torch.tensor(h["nodes"])
        nodes[:, 3] = torch.where(nodes[:, 2] == 2, nodes[:, 3], torch.zeros_like(nodes[:, 3]))
        _inputs[(n, sky)] = (nodes, torch.tensor(h["means3D"]), torch.log(torch.tensor(h["scales"])))
    return _inputs[(n, sky)]


_refs = {}


def _reference(key, nodes, xyz, scaling, root, volume, min_size, tg=TG):
    if key not in _refs:
        _refs[key] = _host_reference(nodes, xyz, scaling, root, volume, tg, min_size)
    return _refs[key]


def _packed_views(xyz, scaling):
    """xyz and scaling as SPTCache lays them out: strided views of one packed pinned host table (spt_cache.py:164-175)."""
    from hlgs_core.spt_cache import NAMES
    widths = dict(xyz=3, f_dc=3, opacity=1, scaling=3, rotation=4, f_rest=45)
    w = [widths[k] for k in NAMES] * 3
    hw = -(-sum(w) // 16) * 16
    host = torch.zeros((xyz.shape[0], hw), dtype=torch.float32, pin_memory=True)
    off = {k: sum(w[:i]) for i, k in enumerate(NAMES)}
    vx, vs = host[:, off["xyz"]:off["xyz"] + 3], host[:, off["scaling"]:off["scaling"] + 3]
    vx.copy_(xyz)
    vs.copy_(scaling)
    assert not vx.is_contiguous() and vx.is_pinned()
    return vx, vs


# ------------------------------------------------------------------------------------------------ 1. the three cases
@pytest.mark.parametrize("layout", ["device", "packed_pinned_views"])
@pytest.mark.parametrize("spheres", [True, False])
@pytest.mark.parametrize("n,sky,volume,min_size", [(3000, 5, 5.0, 20), (6000, 0, 2.0, 50), (2000, 3, 20.0, 10)])
def test_device_build_matches_host_build(n, sky, volume, min_size, spheres, layout):
    nodes, xyz, scaling = _hierarchy(n, sky)
    want = _reference((n, sky, volume, min_size), nodes, xyz, scaling, sky, volume, min_size)
    assert len(want["SPT_root_hierarchy_indices"]) > 3, "the case should build several SPTs"
    if layout == "device":
        args = (nodes.to(DEV), xyz.to(DEV), scaling.to(DEV))
    else:
        args = (nodes,) + _packed_views(xyz, scaling)
    got = spt.build_hierarchical_spt_device(*args, sky, volume, TG, min_size, use_bounding_spheres=spheres)
    assert all(v is None or (v.is_cuda and v.is_contiguous()) for v in got.values())
    _compare(got, want, spheres)


# ------------------------------------------------------------------------------------------------ 2. the fixtures
def _canonical_spts(starts, gidx, smax, smin):
    """Each SPT's entries ordered by (max distance descending, Gaussian index): the fixture's order inside ties of the
    max distance is that of torch's unstable CPU argsort (tests/test_spt_golden.py)."""
    gidx, smax, smin = np.asarray(gidx), np.asarray(smax), np.asarray(smin)
    order = np.concatenate([s + np.lexsort((gidx[s:e], -smax[s:e].astype(np.float64)))
                            for s, e in zip(starts[:-1], starts[1:])]) if len(starts) > 1 else np.zeros(0, np.int64)
    return gidx[order], smax[order], smin[order]


@pytest.mark.parametrize("i", GOLD_CASES)
def test_device_build_matches_reference_run(i):
    sky, volume, tg, min_size, spheres = GOLD[f"params_{i}"]
    sky, min_size, spheres = int(sky), int(min_size), bool(spheres)
    nodes, xyz, log_s = (torch.tensor(GOLD[f"in_{k}_{i}"]) for k in ("nodes", "xyz", "log_scales"))
    want = _host_reference(nodes, xyz, log_s, sky, float(volume), float(tg), min_size)
    got = spt.build_hierarchical_spt_device(nodes, xyz, log_s, sky, float(volume), float(tg), min_size,
                                            use_bounding_spheres=spheres)
    _compare(got, want, spheres)
    got = _np(got)
    starts = GOLD[f"SPT_starts_{i}"]
    a = _canonical_spts(starts, got["SPT_gaussian_indices"], got["SPT_max"], got["SPT_min"])
    b = _canonical_spts(starts, GOLD[f"SPT_gaussian_indices_{i}"], GOLD[f"SPT_max_{i}"], GOLD[f"SPT_min_{i}"])
    np.testing.assert_allclose(got["SPT_max"], GOLD[f"SPT_max_{i}"], rtol=2e-6, atol=0, err_msg="SPT_max sequence")
    np.testing.assert_array_equal(a[0], b[0], err_msg="SPT entries (Gaussian indices within ties)")
    np.testing.assert_allclose(a[1], b[1], rtol=2e-6, atol=0, err_msg="SPT_max")
    np.testing.assert_allclose(a[2], b[2], rtol=2e-6, atol=0, err_msg="SPT_min")
    for k in ("SPT_starts", "upper_tree_nodes", "SPT_root_hierarchy_indices", "upper_tree_xyz", "upper_tree_scaling"):
        np.testing.assert_array_equal(got[k], GOLD[f"{k}_{i}"], err_msg=k)
    np.testing.assert_allclose(got["min_distance_squared"], GOLD[f"min_distance_squared_{i}"], rtol=2e-6, atol=0)
    if spheres:
        np.testing.assert_allclose(got["bounding_sphere_radii"], GOLD[f"bounds_{i}"], rtol=2e-6, atol=0)


# ------------------------------------------------------------------------------------------------ 3. degenerate cuts
def _device(nodes, xyz, scaling, root, volume, min_size, tg=TG, **kw):
    return spt.build_hierarchical_spt_device(nodes.to(DEV), xyz.to(DEV), scaling.to(DEV), root, volume, tg, min_size,
                                             **kw)


def test_every_inner_node_expands():
    nodes, xyz, scaling = _hierarchy(2000, 3)
    want = _reference((2000, 3, 0.0, 10), nodes, xyz, scaling, 3, 0.0, 10)
    got = _device(nodes, xyz, scaling, 3, 0.0, 10)
    _compare(got, want)
    assert got["SPT_starts"].tolist() == [0]
    assert all(got[k].numel() == 0 for k in ("SPT_max", "SPT_min", "SPT_gaussian_indices",
                                             "SPT_root_hierarchy_indices"))
    assert got["upper_tree_nodes"].shape[0] == nodes.shape[0] - 3


def test_root_fails_the_condition():
    nodes, xyz, scaling = _hierarchy(2000, 3)
    want = _reference((2000, 3, 1e30, 10), nodes, xyz, scaling, 3, 1e30, 10)
    got = _device(nodes, xyz, scaling, 3, 1e30, 10)
    _compare(got, want)
    assert got["SPT_starts"].tolist() == [0, nodes.shape[0] - 3]
    assert got["SPT_root_hierarchy_indices"].tolist() == [3] and got["upper_tree_nodes"].shape[0] == 1


def test_no_spt_is_large_enough():
    nodes, xyz, scaling = _hierarchy(2000, 3)
    want = _reference((2000, 3, 20.0, 10 ** 9), nodes, xyz, scaling, 3, 20.0, 10 ** 9)
    got = _device(nodes, xyz, scaling, 3, 20.0, 10 ** 9)
    _compare(got, want)
    assert got["SPT_starts"].tolist() == [0] and got["upper_tree_nodes"].shape[0] == nodes.shape[0] - 3


@pytest.mark.parametrize("sky", [0, 2])
def test_single_leaf(sky):
    nodes = torch.full((sky + 1, 6), -99, dtype=torch.int32)
    nodes[sky] = torch.tensor([0, -1, 0, 0, 0, 0], dtype=torch.int32)
    g = torch.Generator().manual_seed(3)
    xyz, scaling = torch.randn(sky + 1, 3, generator=g), torch.randn(sky + 1, 3, generator=g) - 2
    want = _host_reference(nodes, xyz, scaling, sky, 1.0, TG, 10)
    got = _device(nodes, xyz, scaling, sky, 1.0, 10)
    _compare(got, want)
    assert got["SPT_starts"].tolist() == [0] and got["upper_tree_nodes"].shape[0] == 1


# ------------------------------------------------------------------------------------------------ 4. depth
def _caterpillar(leaves=300):
    """A hierarchy of depth leaves - 1 in make_dynamic_hierarchy's node layout: inner node k has one leaf child and the
    inner node k + 1 (the last one two leaves); which of the two comes first alternates."""
    if "caterpillar" not in _inputs:
        inner = leaves - 1
        G = leaves + inner
        nodes = torch.zeros((G, 6), dtype=torch.int32)
        ids = lambda k: 2 * k  # noqa: E731  inner node k; its leaf is 2 k + 1; the last leaf is G - 1
        for k in range(inner):
            v, leaf = ids(k), 2 * k + 1
            other = ids(k + 1) if k + 1 < inner else G - 1
            first, second = (leaf, other) if k % 2 == 0 else (other, leaf)
            nodes[v, 2], nodes[v, 3] = 2, first
            nodes[first, 4] = second
            for c in (first, second):
                nodes[c, 0], nodes[c, 1] = k + 1, v
        nodes[0, 1] = -1
        leaf_rows = nodes[:, 2] == 0
        nodes[leaf_rows, 5] = torch.arange(int(leaf_rows.sum()), dtype=torch.int32)
        nodes[~leaf_rows, 5] = -1
        g = torch.Generator().manual_seed(300)
        xyz = torch.randn(G, 3, generator=g)
        scaling = torch.randn(G, 3, generator=g) * 0.3 - 1.5
        _inputs["caterpillar"] = (nodes, xyz, scaling)
    return _inputs["caterpillar"]


@pytest.mark.parametrize("volume", [0.0, 1e30])
def test_depth_299(volume):
    """299 levels in the upper walk (volume 0) and in one SPT walk (volume 1e30): no fixed level cap."""
    nodes, xyz, scaling = _caterpillar()
    want = _reference(("caterpillar", volume), nodes, xyz, scaling, 0, volume, 10)
    got = _device(nodes, xyz, scaling, 0, volume, 10)
    _compare(got, want)
    assert int(want["upper_tree_nodes"][:, 0].max()) == (299 if volume == 0.0 else 0)
    assert len(want["SPT_starts"]) == (1 if volume == 0.0 else 2)
    assert spt.last_device_build["host_syncs"] >= 299


# ------------------------------------------------------------------------------------------------ 5. one large SPT
def _exp_safe(log_scales):
    """The nearest float32 values at or above log_scales whose exponential lies within 0.1 ULP of a float32 value, so
    that libm's expf, torch's exp and the device's all round it alike.  Steps of 1, 2 and 3 floats alternate (a fixed
    step can cycle); a value not settled after 400 of them becomes 0, whose exponential is exact."""
    l = log_scales.numpy().copy()
    for k in range(401):
        e = np.exp(l.astype(np.float64))
        r = e / np.exp2(np.frexp(e)[1] - 24.0)
        bad = np.abs(r - np.rint(r)) > 0.1
        if k == 400 or not bad.any():
            break
        for _ in range(1 + k % 3):
            l[bad] = np.nextafter(l[bad], np.float32(np.inf))
    l[bad] = 0.0
    return torch.tensor(l)


def _large_input():
    """The 40,000-leaf hierarchy of make_dynamic_hierarchy with values under which the restatement check can hold on any
    CPU.  With the generator's own values, among 79,999 rows of one SPT some max distances of unrelated nodes are
    neighbouring floats, and the host build and the restatement then order 12 to 78 rows differently, depending on
    the machine: torch's CPU exp and sqrt are not correctly rounded (its sqrt differs from sqrtf on ~0.5 % of these
    rows) and its division by a granularity of 0.02 rounds unlike the host's.  So: positions on a grid of 2 (squared
    distances are small integers, exact in any order), one scale per depth, exp(-0.6 depth) at _exp_safe values, and the
    granularity 2^-6, by which dividing is exact.  The distances then take few values: 79,999 rows share 662 distinct
    sort keys, 107 ULP apart or more (16 asserted), so an error of an ULP cannot reorder them, and the order inside the
    long ties is the walk order, which is what the stable segmented sort has to keep."""
    if "large" not in _inputs:
        nodes, xyz, _ = _hierarchy(40_000, 0)
        scaling = _exp_safe((-0.6 * nodes[:, 0].float())[:, None].repeat(1, 3).contiguous())
        _inputs["large"] = (nodes, torch.round(xyz / 2) * 2, scaling)
    return _inputs["large"]


def test_one_spt_larger_than_a_workgroup_sorts():
    nodes, xyz, scaling = _large_input()
    want = _reference((40_000, 0, 1e30, 20), nodes, xyz, scaling, 0, 1e30, 20, tg=2.0 ** -6)
    assert want["SPT_starts"].tolist() == [0, 79_999]
    keys = np.unique(np.concatenate([want["SPT_max"], want["SPT_min"][want["SPT_min"] > 0]]))
    assert len(np.unique(want["SPT_max"])) > 500  # a real sort, not one long tie
    assert (np.diff(keys.astype(np.float64)) / np.spacing(keys[1:]).astype(np.float64)).min() >= 16
    _compare(_device(nodes, xyz, scaling, 0, 1e30, 20, tg=2.0 ** -6), want)


# ------------------------------------------------------------------------------------------------ 6. after growth
SKY, SPT_ARGS = 5, dict(SPT_Root_Volume=5.0, target_granularity=TG, min_SPT_Size=20)


def _growing_scene():
    """The n = 3000 hierarchy with storage and node rows preallocated to 1.3 x its size, 5 % of the leaves nearly
    transparent (the set-up of tests/test_gpu_mcmc.py).  Built once; callers get clones."""
    if "scene" not in _inputs:
        h = S.make_dynamic_hierarchy(S.make_gaussians(3000, 0, S.make_camera(256, 192), seed=3000), skybox_points=SKY,
                                     seed=3000)
        size = h["nodes"].shape[0]
        cap = int(1.3 * size)
        rng = np.random.default_rng(8)
        nodes = torch.zeros((cap, 6), dtype=torch.int32)
        nodes[:size] = torch.tensor(h["nodes"])
        shapes = dict(xyz=(3,), f_dc=(1, 3), opacity=(1,), scaling=(3,), rotation=(4,), f_rest=(15, 3))
        storage = {k: torch.zeros((cap,) + sh) for k, sh in shapes.items()}
        storage["xyz"][:size] = torch.tensor(h["means3D"])
        storage["scaling"][:size] = torch.log(torch.tensor(h["scales"]))
        storage["rotation"][:size] = torch.tensor(h["rotations"])
        op = torch.tensor(h["opacities"]).clamp(0.01, 0.99)
        storage["opacity"][:size] = torch.log(op / (1 - op))
        leaves = torch.where(nodes[:size, 2] == 0)[0]
        low = leaves[torch.tensor(rng.choice(len(leaves), size=len(leaves) // 20, replace=False))]
        storage["opacity"][low] = float(np.log(0.001 / 0.999))
        _inputs["scene"] = (nodes, storage, size, low)
    nodes, storage, size, low = _inputs["scene"]
    return nodes.clone(), {k: v.clone() for k, v in storage.items()}, size, low


def test_build_after_spawn_and_relocation():
    """Spawned and relocated hierarchies are unbalanced and their depth column is stale: the walks use links only."""
    nodes, storage, size, low = _growing_scene()
    opt = {k: dict(exp_avgs=torch.zeros_like(v), exp_avgs_sqs=torch.zeros_like(v)) for k, v in storage.items()}
    new_size = mcmc.add_new_gs(storage, nodes, size, 10 ** 9, seed=5)
    assert new_size > size
    dead = torch.zeros(new_size, dtype=torch.bool)
    dead[low] = True
    dead &= nodes[:new_size, 2] == 0
    assert mcmc.relocate_gs(storage, opt, nodes, dead, new_size, SKY, seed=5) > 0
    args = (nodes[:new_size], storage["xyz"][:new_size], storage["scaling"][:new_size], SKY, 5.0)
    want = _host_reference(*args, TG, 20)
    assert len(want["SPT_root_hierarchy_indices"]) > 3
    _compare(spt.build_hierarchical_spt_device(*args, TG, 20), want)


def _round(on_device):
    from hlgs_core.spt_cache import SPTCache
    nodes, storage, size, _ = _growing_scene()
    b = spt.build_hierarchical_spt(nodes[:size], storage["xyz"][:size], storage["scaling"][:size], SKY,
                                   *SPT_ARGS.values())
    cache = SPTCache(storage, b, SKY)
    cam = S.make_camera(320, 240, T=np.array([0.0, 0.0, 0.3]))
    cache.step(cam["projmatrix"], cam["campos"])
    new_size = mcmc.densify_round(cache, nodes, size, cap_max=10 ** 9, seed=11, spt_args=SPT_ARGS,
                                  spt_on_device=on_device)
    return cache, nodes, new_size


def test_densify_round_on_device_equals_host_round():
    host, nodes_h, size_h = _round(False)
    dev, nodes_d, size_d = _round(True)
    assert size_d == size_h and torch.equal(nodes_d, nodes_h) and torch.equal(dev.host, host.host)
    # the round's input passes the restatement check
    _host_reference(nodes_h[:size_h], host.storage["xyz"][:size_h].clone(), host.storage["scaling"][:size_h].clone(),
                    SKY, *SPT_ARGS.values())
    assert dev.num_spts == host.num_spts > 3
    for k in ("spt_starts", "spt_gidx", "nodes", "xyz"):
        assert torch.equal(getattr(dev, k), getattr(host, k)), k
    for k in ("spt_max", "spt_min", "min_distance_squared", "bounds"):
        np.testing.assert_allclose(getattr(dev, k).cpu().numpy(), getattr(host, k).cpu().numpy(), rtol=2e-6, atol=0,
                                   err_msg=k)
    assert (dev.cut_order is None) == (host.cut_order is None)
    if dev.cut_order is not None:
        assert torch.equal(dev.cut_order, host.cut_order)


# ------------------------------------------------------------------------------------------------ 7. errors
def _small_tree():
    """A complete binary tree of 15 nodes in breadth-first numbering plus one unused row: 16 rows."""
    nodes = torch.zeros((16, 6), dtype=torch.int32)
    for v in range(15):
        nodes[v, 0] = int(np.log2(v + 1))
        nodes[v, 1] = (v - 1) // 2 if v else -1
        if 2 * v + 2 < 15:
            nodes[v, 2], nodes[v, 3] = 2, 2 * v + 1
            nodes[2 * v + 1, 4] = 2 * v + 2
    g = torch.Generator().manual_seed(16)
    return nodes, torch.randn(16, 3, generator=g), torch.randn(16, 3, generator=g) * 0.3 - 1.0


def _expect_clean_rejection(build, match, syncs=None):
    """The rejected input raises (after `syncs` read-backs, when given), and the next valid build in the same process is
    still right."""
    with pytest.raises(RuntimeError, match=match):
        build()
    assert syncs is None or spt.last_device_build["host_syncs"] == syncs
    nodes, xyz, scaling = _hierarchy(2000, 3)
    want = _reference((2000, 3, 20.0, 10), nodes, xyz, scaling, 3, 20.0, 10)
    _compare(_device(nodes, xyz, scaling, 3, 20.0, 10), want)


@pytest.mark.parametrize("volume", [0.0, 1e30])
def test_first_child_past_the_table_is_rejected_before_any_walk(volume):
    nodes, xyz, scaling = _hierarchy(2000, 3)
    bad = nodes.clone()
    G = bad.shape[0]
    inner = int(torch.where(bad[:, 2] == 2)[0][G // 4])
    bad[inner, 3] = G + 5
    # one read-back, the validation's error word: no walk was launched
    _expect_clean_rejection(lambda: _device(bad, xyz, scaling, 3, volume, 10), "out of range", syncs=1)


@pytest.mark.parametrize("volume", [0.0, 1e30])
def test_link_back_to_the_grandparent_is_rejected(volume):
    """Node 7 gets children: node 1, its grandparent, and node 1's sibling.  Both are in range, so only the bounded walk
    can catch it (the upper walk at volume 0, the SPT walk at volume 1e30)."""
    nodes, xyz, scaling = _small_tree()
    nodes[7, 2], nodes[7, 3] = 2, 1
    _expect_clean_rejection(lambda: _device(nodes, xyz, scaling, 0, volume, 2), "reached twice|does not terminate")


def test_first_child_without_a_sibling_is_rejected():
    nodes, xyz, scaling = _small_tree()
    nodes[3, 4] = 0  # node 1's first child
    _expect_clean_rejection(lambda: _device(nodes, xyz, scaling, 0, 1e30, 2), "binary hierarchy")
    with pytest.raises(RuntimeError, match="binary hierarchy"):
        spt.build_hierarchical_spt(nodes, xyz, scaling, 0, 1e30, TG, 2)
