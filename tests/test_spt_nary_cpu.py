"""The n-ary mode of the SPT path on the CPU: the restatement (tests/spt_nary_ref.py) against a hand-derived tree, the
host build (csrc/spt_build.cpp, build_hierarchical_spt(nary=True)) and the order builder (upper_tree_order(nary=True))
against the restatement on merged scenes, binary equivalence, malformed tables, and the default mode's rejection."""
import numpy as np
import pytest
import torch

import spt_nary_cases as C
import spt_nary_ref as NR
from hlgs_core import spt
from hlgs_core import synthetic as S


def _host(nodes, xyz, scaling, root, volume, tg, min_size, **kw):
    return spt.build_hierarchical_spt(torch.as_tensor(nodes), torch.as_tensor(xyz), torch.as_tensor(scaling), root,
                                      volume, tg, min_size, **kw)


# ------------------------------------------------------------------------------------------------ the hand-derived tree
HAND_UPPER = np.array([[0, -1, 3, 1, 0, 0], [1, 0, 0, 0, 2, 1], [1, 0, 5, 4, 3, 2], [1, 0, 1, 9, 0, 3],
                       [2, 2, 0, -1, 5, 5], [2, 2, 0, -1, 6, 6], [2, 2, 0, -1, 7, 7], [2, 2, 0, -1, 8, 8],
                       [2, 2, 0, -1, 0, 9], [2, 3, 0, -1, 0, 12]], np.int32)


def test_restatement_on_the_hand_derived_tree():
    nodes, xyz, scaling = C.hand()
    r = NR.build_spt_nary(nodes, xyz, scaling, **C.HAND_ARGS)
    # the root and row 2 expand; rows 1 and 3 fail the condition; the five children of row 2 come in list order
    assert r["frontiers"] == [[0], [1, 2, 3], [5, 6, 7, 8, 9]]
    assert r["cut"] == [1, 3, 5, 6, 7, 8, 9]
    # row 1's walk is [1], [4], [10, 11]: 4 entries > 3 and kept; row 3's is [3], [12]: dropped, 12 joins the upper tree
    assert r["SPT_root_hierarchy_indices"].tolist() == [1] and r["dropped"] == [3]
    assert r["SPT_starts"].tolist() == [0, 4]
    assert r["SPT_gaussian_indices"].tolist() == [1, 4, 10, 11]  # max: 1e12, then three ties in walk order
    m1 = np.float32(np.sqrt(np.float32(3) * np.exp(np.float32(-2))) / np.float32(0.5))  # md of row 1
    np.testing.assert_allclose(r["SPT_max"], [1e12, m1, m1, m1], rtol=2e-6)
    np.testing.assert_allclose(r["SPT_min"], [m1, m1, -1e9, -1e9], rtol=2e-6)  # row 4: min(md + 1, parent's min)
    np.testing.assert_array_equal(r["upper_tree_nodes"], HAND_UPPER)
    # leaves 3 x 1; the SPT at row 1: |14 - 10| + 3; row 3: 3 + 2; row 2: 3 + 5; the root: max(7 + 10, 8 + 20, 5 + 10)
    np.testing.assert_array_equal(r["bounding_sphere_radii"], np.float32([28, 7, 8, 5, 3, 3, 3, 3, 3, 3]))
    assert r["min_distance_squared"][0] == np.float32(1e12)
    np.testing.assert_allclose(r["min_distance_squared"][9], m1 * m1, rtol=2e-6)  # the parent of 12 is row 3


def test_restatement_frontiers_cut_and_order_on_the_hand_derived_tree():
    nodes, xyz, _ = C.hand()
    o = NR.order_nary(nodes)
    # rank-major: the rank-0 children of 1, 2, 3, then ranks 1 .. 4 of row 2
    assert o["nodes"].tolist() == [0, 1, 2, 3, 4, 5, 12, 6, 7, 8, 9, 10, 11]
    assert o["level_starts"].tolist() == [0, 1, 4, 11, 13]
    assert o["pos"].tolist() == [0, 1, 5, 11, 2, 6, 12, 7, 8, 9, 10, 3, 4]
    assert o["end"].tolist() == [13, 5, 11, 13, 5, 7, 13, 8, 9, 10, 11, 4, 5]
    cut, states, sizes = NR.upper_tree_cut_nary(nodes, xyz, None, None, None, None, use_frustum=False, use_lod=False)
    assert cut.tolist() == [5, 12, 6, 7, 8, 9, 10, 11] and sizes == [1, 3, 7, 2]
    assert sorted(v for v, s in states.items() if s == 3) == [0, 1, 2, 3, 4]


def test_host_build_on_the_hand_derived_tree():
    nodes, xyz, scaling = C.hand()
    a = C.HAND_ARGS
    got = _host(nodes, xyz, scaling, a["root"], a["volume"], a["tg"], a["min_size"], nary=True)
    assert got.pop("nary") is True and set(got) == set(spt.SPT_KEYS)
    C.compare(got, NR.build_spt_nary(nodes, xyz, scaling, **a))
    np.testing.assert_array_equal(got["upper_tree_nodes"].numpy(), HAND_UPPER)


# ------------------------------------------------------------------------------------------------ merged scenes
@pytest.mark.parametrize("name,sky,volume,min_size", C.CASES)
def test_host_build_matches_the_restatement(name, sky, volume, min_size):
    nodes, xyz, scaling = C.scene(name, sky)
    want = C.reference(name, sky, volume, min_size)
    got = _host(nodes, xyz, scaling, sky, volume, C.TG, min_size, nary=True)
    assert got["nary"] is True
    C.compare(got, want)
    nos = _host(nodes, xyz, scaling, sky, volume, C.TG, min_size, use_bounding_spheres=False, nary=True)
    C.compare(nos, want, spheres=False)


@pytest.mark.parametrize("name", ["k3", "k8"])
def test_merged_scenes_are_not_binary(name):
    cc = C.scene(name)[0][:, 2]
    assert (cc == 1).sum() >= 20 and (cc >= 3).sum() >= 10
    leaves = np.where(cc == 0)[0]
    assert (C.scene(name)[0][leaves, 3] == leaves + 1).all()  # the merger's leaves: first_child = id + 1


@pytest.mark.parametrize("name,sky,volume,min_size", C.MERGED_CASES)
def test_scene_properties_from_the_restatement(name, sky, volume, min_size):
    r = C.reference(name, sky, volume, min_size)
    assert len(r["SPT_root_hierarchy_indices"]) >= 4
    assert len(r["dropped"]) >= 1
    assert any(1 in s and max(s) >= 3 for s in r["spt_child_counts"]), "a kept SPT with a 1-child and a 3+-child node"
    assert (r["upper_tree_nodes"][:, 2] >= 3).any()


# ------------------------------------------------------------------------------------------------ binary equivalence
def _binary_hierarchy(n, sky):
    """The synthetic binary hierarchy of tests/test_gpu_spt_build.py::test_device_build_matches_host_build."""
    h = S.make_dynamic_hierarchy(S.make_gaussians(n, 0, S.make_camera(256, 192), seed=n), skybox_points=sky, seed=n)
    nodes = torch.tensor(h["nodes"])
    nodes[:, 3] = torch.where(nodes[:, 2] == 2, nodes[:, 3], torch.zeros_like(nodes[:, 3]))
    return nodes, torch.tensor(h["means3D"]), torch.log(torch.tensor(h["scales"]))


BINARY_CASES = [(3000, 5, 5.0, 20), (6000, 0, 2.0, 50), (2000, 3, 20.0, 10)]


@pytest.mark.parametrize("n,sky,volume,min_size", BINARY_CASES)
def test_nary_mode_equals_binary_mode_bit_for_bit(n, sky, volume, min_size):
    nodes, xyz, scaling = _binary_hierarchy(n, sky)
    for spheres in (True, False):
        a = spt.build_hierarchical_spt(nodes, xyz, scaling, sky, volume, C.TG, min_size, spheres)
        b = spt.build_hierarchical_spt(nodes, xyz, scaling, sky, volume, C.TG, min_size, spheres, nary=True)
        assert set(a) == set(spt.SPT_KEYS) and b.pop("nary") is True
        assert len(a["SPT_root_hierarchy_indices"]) > 3
        C.compare(b, C.to_numpy(a), spheres, exact_floats=True)
    oa = spt.upper_tree_order(a["upper_tree_nodes"], device="cpu")
    ob = spt.upper_tree_order(a["upper_tree_nodes"], device="cpu", nary=True)
    assert oa is not None and torch.equal(oa, ob)


# ------------------------------------------------------------------------------------------------ the order builder
def _unpack(blob):
    b = blob.numpy()
    M, levels = int(b[0]), int(b[1])
    fn = b[80:]  # HLGS_CUT_ORDER_HEADER
    return dict(nodes=fn[:M], level_starts=b[4:4 + levels + 1], pos=fn[M:2 * M] & 0xffff,
                end=(fn[M:2 * M].astype(np.int64) >> 16) & 0xffff, N=int(b[3]))


@pytest.mark.parametrize("case", [None] + C.CASES[:3])
def test_order_builder_matches_the_restatement(case):
    un = C.hand()[0] if case is None else C.reference(*case)["upper_tree_nodes"]
    blob = spt.upper_tree_order(torch.tensor(un), device="cpu", nary=True)
    want = NR.order_nary(un)
    assert blob is not None and want is not None
    got = _unpack(blob)
    assert got["N"] == len(un)
    for k in ("nodes", "level_starts", "pos", "end"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


def _star(n):
    nd = np.zeros((n + 1, 6), np.int32)
    nd[0] = (0, -1, n, 1, 0, 0)
    for i in range(1, n + 1):
        nd[i] = (1, 0, 0, i + 1, i + 1 if i < n else 0, 0)
    return nd


def _chain(depth):
    """depth one-child nodes under each other, then a leaf."""
    nd = np.zeros((depth + 1, 6), np.int32)
    for i in range(depth + 1):
        nd[i] = (i, i - 1, 1 if i < depth else 0, i + 1, 0, 0)
    return nd


def test_order_builder_limits():
    assert spt.upper_tree_order(torch.tensor(_star(65534)), device="cpu", nary=True) is not None  # 65,535 entries
    assert spt.upper_tree_order(torch.tensor(_star(65535)), device="cpu", nary=True) is None
    assert spt.upper_tree_order(torch.tensor(_chain(63)), device="cpu", nary=True) is not None  # 64 levels
    assert spt.upper_tree_order(torch.tensor(_chain(64)), device="cpu", nary=True) is None
    for nd in C.malformed().values():  # not a tree: not usable, and no error
        assert spt.upper_tree_order(torch.tensor(nd), device="cpu", nary=True) is None


# ------------------------------------------------------------------------------------------------ malformed tables
@pytest.mark.parametrize("name", sorted(C.malformed()))
def test_malformed_table_is_rejected_and_the_next_build_is_right(name):
    _, xyz, scaling = C.hand()
    a = C.HAND_ARGS
    with pytest.raises(ValueError):
        NR.validate(C.malformed()[name], 0)
    with pytest.raises(RuntimeError):
        _host(C.malformed()[name], xyz, scaling, a["root"], a["volume"], a["tg"], a["min_size"], nary=True)
    got = _host(C.HAND_NODES, xyz, scaling, a["root"], a["volume"], a["tg"], a["min_size"], nary=True)
    np.testing.assert_array_equal(got["upper_tree_nodes"].numpy(), HAND_UPPER)
    assert got["SPT_gaussian_indices"].tolist() == [1, 4, 10, 11]


def test_default_mode_still_rejects_a_one_child_node():
    nodes, xyz, scaling = C.hand()
    a = C.HAND_ARGS
    with pytest.raises(RuntimeError, match="binary hierarchy"):
        _host(nodes, xyz, scaling, a["root"], a["volume"], a["tg"], a["min_size"])
    with pytest.raises(RuntimeError, match="binary hierarchy"):
        _host(nodes, xyz, scaling, a["root"], a["volume"], a["tg"], a["min_size"], nary=False)
