"""CPU checks around the GPU hierarchy creator (hlgs_core.hierarchy, csrc/hier_build.hip): the numpy restatement the
GPU tests compare against (tests/hier_build_ref.py) on trees derived by hand, the closed-form node table against the
writer's recursion, the aligner's 24-candidate choice, and the public surface without a device."""
import numpy as np
import pytest
import torch

import hier_build_ref as R


def _line(xs, axis=0, scale=0.01):
    """Gaussians on one coordinate axis at the given coordinates: identity rotation (unnormalised), one scale."""
    n = len(xs)
    xyz = np.zeros((n, 3), np.float32)
    xyz[:, axis] = xs
    return dict(xyz=xyz, shs=np.arange(3 * n, dtype=np.float32).reshape(n, 3),
                opacity=np.full(n, 0.5, np.float32), scales=np.full((n, 3), scale, np.float32),
                rotations=np.tile(np.array([[2.0, 0, 0, 0]], np.float32), (n, 1)))


def test_one_gaussian_is_one_leaf_row():
    sc = _line([3.0])
    out = R.build_ref(sc)
    np.testing.assert_array_equal(out["nodes"], [[0, -1, 0, 1, 0, 0]])
    np.testing.assert_array_equal(out["pos"], sc["xyz"])
    np.testing.assert_array_equal(out["rot"], [[1, 0, 0, 0]])
    np.testing.assert_array_equal(out["log_scales"], np.log(sc["scales"]))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_two_gaussians_by_hand(dtype):
    """Two spheres of radius 0.5 and opacity 0.5 at x = -1 and +1: w = 0.5 * 0.75 each, a = 1/2, the mean at 0,
    cov = diag(0.25 + 1, 0.25, 0.25), scales sqrt of (0.25, 0.25, 1.25) ascending, opacity 0.75 / surface."""
    sc = _line([1.0, -1.0], scale=0.5)
    sc["shs"] = np.array([[1, 2, 3], [3, 4, 5]], np.float32)
    out = R.build_ref(sc, dtype)
    np.testing.assert_array_equal(out["nodes"], [[0, -1, 2, 1, 0, -1], [1, 0, 0, 2, 2, 1], [1, 0, 0, 3, 0, 0]])
    np.testing.assert_array_equal(out["pos"], [[0, 0, 0], [-1, 0, 0], [1, 0, 0]])
    np.testing.assert_array_equal(out["shs"], [[2, 3, 4], [3, 4, 5], [1, 2, 3]])
    np.testing.assert_array_equal(out["cov"][0], [1.25, 0, 0, 0.25, 0, 0.25])
    s = np.sqrt(1.25)
    np.testing.assert_allclose(out["scale"][0], [0.5, 0.5, s], rtol=1e-6)
    np.testing.assert_allclose(out["alpha"], [0.75 / (0.25 + 0.5 * s + 0.5 * s), 0.5, 0.5], rtol=1e-6)
    np.testing.assert_allclose(R.rebuilt_cov(out["rot"], out["log_scales"])[0], np.diag([1.25, 0.25, 0.25]),
                               atol=1e-6)
    # the children are aligned with the root: their axes are signed permutations of the identity, scales unchanged
    for row in (1, 2):
        m = R.matrix_from_quat(out["rot"][row])
        np.testing.assert_allclose(np.abs(m).sum(axis=0), 1, atol=1e-6)
        assert (m * R.matrix_from_quat(out["rot"][0])).sum() > 2.999


def test_three_and_five_gaussians_by_hand():
    out = R.build_ref(_line([2.0, 0.0, 1.0]))
    np.testing.assert_array_equal(out["nodes"], [[0, -1, 2, 1, 0, -1], [1, 0, 0, 2, 2, 1], [1, 0, 2, 3, 0, -1],
                                                 [2, 2, 0, 4, 4, 2], [2, 2, 0, 5, 0, 0]])
    # 5 -> (2, 3); 3 -> (1, 2): rows by x are 1, 3 | 4 | 2, 0
    out = R.build_ref(_line([4.0, 0.0, 3.0, 1.0, 2.0], axis=1))
    np.testing.assert_array_equal(out["nodes"], [[0, -1, 2, 1, 0, -1], [1, 0, 2, 2, 4, -1], [2, 1, 0, 3, 3, 1],
                                                 [2, 1, 0, 4, 0, 3], [1, 0, 2, 5, 0, -1], [2, 4, 0, 6, 6, 4],
                                                 [2, 4, 2, 7, 0, -1], [3, 6, 0, 8, 8, 2], [3, 6, 0, 9, 0, 0]])
    leaf = out["nodes"][:, R.CHILD_COUNT] == 0
    np.testing.assert_array_equal(out["pos"][leaf, 1], [0, 1, 2, 3, 4])


def test_axis_and_ties_by_hand():
    # equal extents on x and y: the first axis wins; equal coordinates: the lower row goes left; -0.0 ties with +0.0
    sc = _line([0.0, 0.0, 0.0, 0.0])
    sc["xyz"][:, 0] = [1, -0.0, 1, 0.0]
    sc["xyz"][:, 1] = [0, 1, 1, 0]
    out = R.build_ref(sc)
    leaf = out["nodes"][:, R.CHILD_COUNT] == 0
    # x: rows 1, 3 (both zero, by row) | 0, 2; then each pair splits by y (the only extent left beyond the radius)
    np.testing.assert_array_equal(out["nodes"][leaf, R.MAX_SIDE], [3, 1, 0, 2])
    # all positions equal: every extent is equal, axis 0, all keys tie, rows in order
    out = R.build_ref(_line([7.0] * 6))
    leaf = out["nodes"][:, R.CHILD_COUNT] == 0
    np.testing.assert_array_equal(out["nodes"][leaf, R.MAX_SIDE], np.arange(6))


def test_closed_form_node_table_matches_the_writer():
    rng = np.random.default_rng(5)
    for n in range(1, 301):
        sc = _line(rng.permutation(n).astype(np.float32))
        root = R.kd_tree(sc["xyz"], sc["scales"], np.arange(n))
        nodes, order = [[0, -1, 0, 0, 0, 0]], []

        def rec(node, nid, depth):  # writer.cpp:99-171 without the rows
            nodes[nid][R.MAX_SIDE] = 0 if node.leaf >= 0 else -1
            nodes[nid][R.FIRST_CHILD] = len(nodes)
            nodes[nid][R.CHILD_COUNT] = len(node.children)
            nodes[nid][R.DEPTH] = depth
            if node.leaf >= 0:
                order.append((nid, node.leaf))
            for k, c in enumerate(node.children):
                nodes.append([0, nid, 0, 0, 0, 0])
                cid = len(nodes) - 1
                rec(c, cid, depth + 1)
                nodes[cid][R.NEXT_SIBLING] = len(nodes) if k == 0 else 0

        rec(root, 0, 0)
        closed, leafpos = R.closed_form_nodes(n)
        np.testing.assert_array_equal(closed, np.array(nodes, np.int32), err_msg=f"N = {n}")
        # leaves from the left are the rows in coordinate order, at the positions the closed form gives them
        ids = np.array([i for i, _ in order])
        np.testing.assert_array_equal(leafpos[ids], np.arange(n))
        np.testing.assert_array_equal(sc["xyz"][[r for _, r in order], 0], np.arange(n))


def test_aligner_picks_the_first_best_of_24_candidates():
    eye = np.eye(3, dtype=np.float32)
    rz = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], np.float32)  # columns (0,1,0), (-1,0,0), (0,0,1)
    i, j, k, test = R.best_candidate(rz, eye)
    assert (i, j, k) == (1, 0, 2)
    np.testing.assert_array_equal(test, eye)
    # 24 of the 48 signed permutations are proper; each scores 3 against itself and less against any other
    n = 0
    for p in ([0, 1, 2], [0, 2, 1], [1, 0, 2], [1, 2, 0], [2, 0, 1], [2, 1, 0]):
        for state in range(8):
            ref = eye[:, p] * np.array([-1 if state & (1 << w) else 1 for w in range(3)], np.float32)
            if R.col_det(ref) < 0:
                continue
            n += 1
            _, _, _, test = R.best_candidate(eye, ref)
            np.testing.assert_array_equal(test, ref)
    assert n == 24
    # ties keep the first candidate in the loop order (i, j, k, state): the score must be strictly greater
    only_xx = np.zeros((3, 3), np.float32)
    only_xx[0, 0] = 1
    i, j, k, test = R.best_candidate(eye, only_xx)
    assert (i, j, k) == (0, 1, 2)
    np.testing.assert_array_equal(test, eye)
    # no candidate above 0: unchanged (the reference reads uninitialised indices)
    assert R.best_candidate(eye, np.zeros((3, 3), np.float32)) is None


def test_filter_restatement():
    sc = R.make_scene("random", 12, 3)
    sc["opacity"][1] = np.inf
    sc["opacity"][2] = np.nan
    sc["opacity"][3] = 0
    sc["scales"][4, 1] = 10.5
    sc["scales"][5, 2] = np.nan
    sc["rotations"][6, 0] = np.nan
    sc["xyz"][7, 1] = np.nan
    sc["shs"][8, 2] = np.nan
    sc["xyz"][9, 0] = np.inf  # kept: only NaN positions are dropped
    sc["scales"][10, 0] = 10.0  # kept: the test is > 10
    np.testing.assert_array_equal(R.valid_mask_ref(sc), [1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1])


def test_public_functions_exist_and_raise_without_a_gpu():
    import gaussian_hierarchy as GH
    from hlgs_core import _lib as L
    from hlgs_core import hierarchy as H
    assert GH.create_dynamic_hierarchy is H.build_dynamic_hierarchy
    assert GH.valid_gaussian_mask is H.valid_gaussian_mask
    assert {"create_dynamic_hierarchy", "valid_gaussian_mask"} <= set(GH.__all__)
    lib = L.load()
    assert H.LDS_CAP == 2048 and lib.hlgs_hier_scratch_size(H.LDS_CAP + 1) > lib.hlgs_hier_scratch_size(H.LDS_CAP)
    # N < 1 and N above HLGS_HIER_MAX_N are argument errors before anything is launched
    one = torch.zeros(4)
    for n in (0, -1, H.MAX_N + 1):
        assert lib.hlgs_hier_build(n, 3, *[L.ptr(one)] * 12, 0x3f, None) == 1
        assert lib.hlgs_hier_valid_mask(n, 3, *[L.ptr(one)] * 6, None) == 1
    e = lambda *s: torch.zeros(s)  # noqa: E731
    with pytest.raises(ValueError, match="N = 0"):
        H.build_dynamic_hierarchy(e(0, 3), e(0, 16, 3), e(0, 1), e(0, 3), e(0, 4))
    with pytest.raises(ValueError, match="scales must hold"):
        H.build_dynamic_hierarchy(e(2, 3), e(2, 16, 3), e(2, 1), e(2, 2), e(2, 4))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="HIP device"):
            H.build_dynamic_hierarchy(e(2, 3), e(2, 16, 3), e(2, 1), e(2, 3), e(2, 4))
        with pytest.raises(RuntimeError, match="HIP device"):
            H.valid_gaussian_mask(e(2, 3), e(2, 16, 3), e(2, 1), e(2, 3), e(2, 4))
