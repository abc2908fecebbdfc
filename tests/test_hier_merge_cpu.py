"""CPU checks around the GPU chunk merger (hlgs_core.hierarchy.merge_dynamic_hierarchies, csrc/hier_merge.hip): the
recursive numpy restatement the GPU tests compare against (tests/hier_merge_ref.py) on trees derived by hand, the
closed form against the recursion on every scene kind, the weight against synthetic.chunk_weight, and the conditions
the scenes must meet for the GPU tests to mean something."""
import functools

import numpy as np
import pytest
import torch

import hier_merge_ref as R
from hlgs_core import synthetic as S

F = np.float32
CEN2 = np.array([(0, 0, 0), (4, 0, 0)], F)
NEAR, FAR = (0.5, 0, 0), (3.5, 0, 0)  # w = 1 and w = 0 for chunk 0 of CEN2


def _hand(links, where):
    """A chunk from (parent, children) links and one position per row; floats that tell the rows apart."""
    n = len(where)
    nodes = np.zeros((n, 6), np.int32)
    nodes[0, R.PARENT] = -1
    for p, kids in links.items():
        nodes[p, R.CHILD_COUNT], nodes[p, R.FIRST_CHILD] = len(kids), kids[0]
        for a, b in zip(kids, kids[1:] + [0]):
            nodes[a, R.PARENT], nodes[a, R.DEPTH], nodes[a, R.NEXT_SIBLING] = p, nodes[p, R.DEPTH] + 1, b
    pos = np.array(where, F)
    row = np.arange(n, dtype=F)[:, None]
    return pos, np.tile(row + 0.25, (1, 3)).reshape(n, 1, 3), row * 0 + 0.5, np.tile(row - 3, (1, 3)), \
        np.tile(row + 1, (1, 4)), nodes


def _merged(chunk, centers=CEN2):
    # the second chunk: one far-away root that keeps only itself
    other = _hand({}, [tuple(centers[1])])
    return R.merge_ref([chunk, other], centers)


def test_one_node():
    out = R.merge_ref([_hand({}, [(9, 9, 9)])], np.zeros((1, 3), F))
    np.testing.assert_array_equal(out["nodes"], [[0, -1, 1, 1, 0, -1], [1, 0, 0, 2, 0, 0]])
    np.testing.assert_array_equal(out["pos"], np.zeros((2, 3), F))  # the chunk root sits at the centre, and so the root
    np.testing.assert_array_equal(out["alpha"], F([0.5, 0.5]))
    np.testing.assert_array_equal(out["log_scales"][0], np.full(3, F(np.log(1e4)), F))
    np.testing.assert_array_equal(out["rot"][0], F([1, 0, 0, 0]))
    np.testing.assert_array_equal(out["shs"][0], out["shs"][1])
    np.testing.assert_array_equal(out["chunk_roots"], [1])


def test_two_nodes_dropped_leaf():
    out = _merged(_hand({0: [1]}, [NEAR, FAR]))
    np.testing.assert_array_equal(out["nodes"], [[0, -1, 2, 1, 0, -1], [1, 0, 0, 2, 2, -1], [1, 0, 0, 3, 0, 0]])
    np.testing.assert_array_equal(out["chunk_roots"], [1, 2])


def test_three_nodes_dropped_leaf():
    out = _merged(_hand({0: [1, 2]}, [NEAR, FAR, NEAR]))
    np.testing.assert_array_equal(out["nodes"], [[0, -1, 2, 1, 0, -1], [1, 0, 1, 2, 3, -1], [2, 1, 0, 3, 0, 0],
                                                 [1, 0, 0, 4, 0, 1]])
    np.testing.assert_array_equal(out["pos"][2], F(NEAR))
    np.testing.assert_array_equal(out["log_scales"][2], F([-1, -1, -1]))  # input row 2


def test_five_nodes_dropped_interior_with_both_children_kept():
    # 0 -> (1 dropped -> (2, 3), 4): 2 and 3 take 1's place in front of 4
    out = _merged(_hand({0: [1, 4], 1: [2, 3]}, [NEAR, FAR, NEAR, NEAR, NEAR]))
    np.testing.assert_array_equal(out["nodes"], [[0, -1, 2, 1, 0, -1], [1, 0, 3, 2, 5, -1], [2, 1, 0, 3, 3, 0],
                                                 [2, 1, 0, 4, 4, 1], [2, 1, 0, 5, 0, 2], [1, 0, 0, 6, 0, 3]])
    np.testing.assert_array_equal(out["rot"][1:5, 0], F([1, 3, 4, 5]))  # input rows 0, 2, 3, 4


def test_five_nodes_dropped_interior_under_dropped_interior():
    # 0 -> 1 dropped -> (2 dropped -> (3, 4)): 3 and 4 hang on the root
    out = _merged(_hand({0: [1], 1: [2], 2: [3, 4]}, [NEAR, FAR, FAR, NEAR, NEAR]))
    np.testing.assert_array_equal(out["nodes"][:4], [[0, -1, 2, 1, 0, -1], [1, 0, 2, 2, 4, -1], [2, 1, 0, 3, 3, 0],
                                                     [2, 1, 0, 4, 0, 1]])


def test_five_nodes_kept_interior_with_nothing_below():
    # 0 -> (1 kept -> (2, 3) dropped, 4): 1 stays with no children and is no leaf of its input
    out = _merged(_hand({0: [1, 4], 1: [2, 3]}, [NEAR, NEAR, FAR, FAR, NEAR]))
    np.testing.assert_array_equal(out["nodes"][:4], [[0, -1, 2, 1, 0, -1], [1, 0, 2, 2, 4, -1], [2, 1, 0, 3, 3, -1],
                                                     [2, 1, 0, 4, 0, 0]])


def test_weight_scales_opacity_and_nan_drops():
    band = (2.0, 0, 0)  # equidistant: w = a d + b = 0.5 up to rounding
    ch = _hand({0: [1, 2]}, [NEAR, band, (np.nan, 0, 0)])
    out = _merged(ch)
    w = R.weights(np.array([band], F), 0, CEN2)[0]
    assert 0.49 < w < 0.51
    assert len(out["nodes"]) == 4 and out["alpha"][2] == F(0.5) * w
    with pytest.raises(ValueError):
        R.merge_ref([_hand({}, [NEAR])], np.array([[np.nan, 0, 0]], F))


SCENES = [("uniform", 1000, 2, False), ("uniform", 1000, 3, True), ("bisector", 1000, 2, False),
          ("all_far", 200, 2, False), ("chain", 300, 2, False), ("wide", 300, 3, True), ("appended", 1000, 3, False),
          ("appended", 1000, 2, True), ("uniform", (1, 65, 1000), 3, False), ("uniform", 3, 1, False)]


@pytest.mark.parametrize("kind,L,K,shuffle", SCENES, ids=[f"{k}-{l}-K{K}-{'sh' if s else 'pre'}" for k, l, K, s in SCENES])
def test_closed_form_equals_recursion(kind, L, K, shuffle):
    chunks, cen = R.make_scene(kind, L, K, shuffle=shuffle)
    ref = R.merge_ref(chunks, cen)
    nodes, roots, src = R.closed_form_nodes(chunks, cen)
    np.testing.assert_array_equal(nodes, ref["nodes"])
    np.testing.assert_array_equal(roots, ref["chunk_roots"])
    for k, ch in enumerate(chunks):  # the rows arrive where the closed form says
        mine = np.where(src[:, 0] == k)[0]
        np.testing.assert_array_equal(ref["rot"][mine], R.flat(ch)[4][src[mine, 1]])


def test_shuffling_does_not_change_the_result():
    chunks, cen = R.make_scene("appended", 200, 2)
    a = R.merge_ref(chunks, cen)
    b = R.merge_ref([R.shuffled(ch, 5) for ch in chunks], cen)
    for key in a:
        np.testing.assert_array_equal(a[key], b[key])


@pytest.mark.parametrize("K", [1, 2, 3, 8])
def test_weight_equals_chunk_weight(K):
    cen = R.centers_for(K)
    rng = np.random.default_rng(K)
    pos = rng.uniform(-4, 8, (20000, 3)).astype(F)
    for k in range(K):
        np.testing.assert_array_equal(R.weights(pos, k, cen), S.chunk_weight(pos, k, cen))


@functools.lru_cache(maxsize=None)
def _stats(kind, L, K):
    chunks, cen = R.make_scene(kind, L, K)
    return [R.splice_stats(ch, k, cen) for k, ch in enumerate(chunks)]


@pytest.mark.parametrize("K", [2, 3])
def test_uniform_scene_exercises_every_branch(K):
    for st in _stats("uniform", 1000, K):
        print(st)
        assert st["one"] >= 0.60 and st["band"] >= 0.03 and st["zero"] >= 0.10
        assert st["splices"] >= 20 and st["widest"] > 2


def test_bisector_scene_fills_the_band():
    for st in _stats("bisector", 1000, 2):
        print(st)
        assert st["band"] >= 0.20


def test_other_scenes_are_what_they_say():
    chunks, cen = R.make_scene("all_far", 200, 2)
    ref = R.merge_ref(chunks, cen)
    assert len(ref["nodes"]) == 3 and ref["nodes"][1, R.CHILD_COUNT] == 0
    chunks, _ = R.make_scene("chain", 300, 2)
    assert chunks[0][5][:, R.DEPTH].max() == 300
    chunks, _ = R.make_scene("wide", 300, 2)
    assert chunks[0][5][0, R.CHILD_COUNT] == 300
    chunks, _ = R.make_scene("appended", 1000, 2)
    nd = chunks[0][5]
    assert len(nd) > 1999 + 90 and np.all(nd[1999:, R.FIRST_CHILD] == 0) and np.any(nd[:1999, R.FIRST_CHILD] >= 1999)


def test_public_functions_exist_and_raise_without_a_gpu():
    import gaussian_hierarchy as GH
    from hlgs_core import _lib as L
    from hlgs_core import hierarchy as H
    assert GH.merge_dynamic_hierarchies is H.merge_dynamic_hierarchies
    assert GH.merge_hierarchy_files is H.merge_hierarchy_files
    assert {"merge_dynamic_hierarchies", "merge_hierarchy_files"} <= set(GH.__all__)
    lib = L.load()
    assert lib.hlgs_hier_merge_scratch_size(1000) > lib.hlgs_hier_merge_scratch_size(10) >= 4 * (8 + 2048)
    # argument errors, before anything is launched
    one = torch.zeros(64)
    for n in (0, -1, (1 << 30) + 1):
        assert lib.hlgs_hier_merge_plan(n, 0, 1, *[L.ptr(one)] * 3, 0.05, L.ptr(one), 3, None) == 1
    for k, K in ((1, 1), (-1, 2), (0, 0)):
        assert lib.hlgs_hier_merge_plan(4, k, K, *[L.ptr(one)] * 3, 0.05, L.ptr(one), 3, None) == 1
    assert lib.hlgs_hier_merge_root(0, 3, 5, *[L.ptr(one)] * 2, 1e4, *[L.ptr(one)] * 6, None) == 1
    chunks, cen = R.make_scene("uniform", 3, 2)
    t = lambda ch: tuple(torch.tensor(a) for a in ch)  # noqa: E731
    with pytest.raises(ValueError, match="at least one chunk"):
        H.merge_dynamic_hierarchies([], np.zeros((0, 3), F))
    with pytest.raises(ValueError, match="centers must have"):
        H.merge_dynamic_hierarchies([t(chunks[0])], cen)
    with pytest.raises(ValueError, match="not finite"):
        H.merge_dynamic_hierarchies([t(ch) for ch in chunks], np.full_like(cen, np.inf))
    with pytest.raises(ValueError, match="one SH width"):
        H.merge_dynamic_hierarchies([t(chunks[0]), t(R.make_scene("uniform", 3, 2, shf=12)[0][1])], cen)
    with pytest.raises(ValueError, match="rot must hold"):
        H.merge_dynamic_hierarchies([t(chunks[0][:4] + (chunks[0][4][:, :3], chunks[0][5])), t(chunks[1])], cen)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="HIP device"):
            H.merge_dynamic_hierarchies([t(ch) for ch in chunks], cen)
