"""Inputs shared by tests/test_spt_nary_cpu.py and tests/test_gpu_spt_nary.py: the merged scenes (the CPU merger of
tests/hier_merge_ref.py), the hand-derived 13-row tree, and the restatement's results, each computed once."""
import numpy as np
import torch

import hier_merge_ref as HM
import spt_nary_ref as NR

TG = 0.02
INTS = ("SPT_starts", "SPT_gaussian_indices", "SPT_root_hierarchy_indices", "upper_tree_nodes")
EXACT = INTS + ("upper_tree_xyz", "upper_tree_scaling")
CLOSE = ("SPT_max", "SPT_min", "min_distance_squared", "bounding_sphere_radii")
KEYS = EXACT + CLOSE

# name -> (kind, leaves per chunk, chunks, seed)
SCENES = {"k3": ("uniform", 700, 3, 1), "k8": ("uniform", 2000, 8, 0), "wide": ("wide", 40, 3, 0),
          "chain": ("chain", 30, 3, 0)}
# (scene, skybox rows, SPT_Root_Volume, min_SPT_Size): the volumes were chosen on the CPU so that the host build and
# the restatement agree on every integer (no decision within an exp rounding of a tie) and the scene properties of
# test_spt_nary_cpu.py hold
CASES = [("k3", 0, 2.5e-5, 10), ("k8", 0, 2.5e-5, 10), ("k8", 0, 1e-4, 20), ("wide", 0, 2.5e-5, 10),
         ("chain", 0, 2.5e-5, 10), ("k3", 4, 2.5e-5, 10)]
MERGED_CASES = CASES[:3]
# only the scene root expands: every chunk is one SPT of ~2,300 entries, more than a workgroup
BIG_SPT_CASE = ("k8", 0, 1e11, 10)
CASES.append(BIG_SPT_CASE)
# the cut tests' ring of six cameras around the K = 8 scene: each camera's distance from the centre and the distance
# multiplier of its view, then the two unions (test_gpu_spt_nary.py).  A small multiplier walks deep (wide levels,
# many leaves), a large one stops early (condition-false nodes); near cameras cull, far ones see the whole scene.
CUT_RADII = (5.0, 10.0, 5.0, 10.0, 3.0, 14.0)
CUT_VIEWS = [((k,), dm) for k, dm in enumerate((0.02, 0.02, 0.02, 0.02, 0.2, 0.2))] + [((0, 3), 0.02),
                                                                                       ((0, 1, 2, 4), 0.05)]

_scenes, _refs = {}, {}


def with_skybox(nodes, xyz, scaling, sky):
    """sky rows without a hierarchy in front (scene/gaussian_model.py:1059-1065): every link shifts by sky."""
    if not sky:
        return nodes, xyz, scaling
    nd = nodes.copy()
    nd[:, 3] += sky
    nd[:, 1] += sky
    nd[nd[:, 4] > 0, 4] += sky
    nd[0, 1] = -1
    rng = np.random.default_rng(sky)
    return (np.concatenate([np.full((sky, 6), -99, np.int32), nd]),
            np.concatenate([rng.normal(0, 50, (sky, 3)).astype(np.float32), xyz]),
            np.concatenate([np.full((sky, 3), 0.7, np.float32), scaling]))


def scene(name, sky=0):
    """(nodes, xyz, log-scales) of a merged scene, as numpy arrays."""
    if (name, sky) not in _scenes:
        kind, L, K, seed = SCENES[name]
        chunks, centers = HM.make_scene(kind, L, K, seed=seed)
        m = HM.merge_ref(chunks, centers)
        _scenes[(name, sky)] = with_skybox(m["nodes"].astype(np.int32), m["pos"].astype(np.float32),
                                           m["log_scales"].astype(np.float32), sky)
    return _scenes[(name, sky)]


def chunks_of(name):
    kind, L, K, seed = SCENES[name]
    return HM.make_scene(kind, L, K, seed=seed)


def reference(name, sky, volume, min_size):
    """The restatement's build of a case (root = sky, with bounding spheres)."""
    key = (name, sky, volume, min_size)
    if key not in _refs:
        nodes, xyz, scaling = scene(name, sky)
        _refs[key] = NR.build_spt_nary(nodes, xyz, scaling, sky, volume, TG, min_size)
    return _refs[key]


def tensors(name, sky=0):
    return tuple(torch.tensor(a) for a in scene(name, sky))


def to_numpy(d):
    return {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else v) for k, v in d.items()}


def compare(got, want, spheres=True, exact_floats=False):
    """Integers and copied rows exact; distances at rtol 2e-6, the bound of tests/test_spt_build.py:30."""
    got = to_numpy(got)
    for k in EXACT:
        assert got[k].shape == want[k].shape, (k, got[k].shape, want[k].shape)
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    for k in CLOSE:
        if k == "bounding_sphere_radii" and not spheres:
            assert got[k] is None
            continue
        assert got[k].shape == want[k].shape, k
        if exact_floats:
            np.testing.assert_array_equal(got[k], want[k], err_msg=k)
        else:
            np.testing.assert_allclose(got[k], want[k], rtol=2e-6, atol=0, err_msg=k)


# ---------------------------------------------------------------------------------------------------------------
# The hand-derived tree: 13 rows {depth, parent, child_count, first_child, next_sibling, -}; the root has 3 children,
# row 1 has one child, row 2 has five, row 3 has one; leaves carry first_child = id + 1 (which is not read).
#        0
#      / | \
#     1  2  3          1 -> 4 -> (10, 11);  2 -> (5, 6, 7, 8, 9);  3 -> 12
HAND_NODES = np.array([
    [0, -1, 3, 1, 0, 0],
    [1, 0, 1, 4, 2, 0],
    [1, 0, 5, 5, 3, 0],
    [1, 0, 1, 12, 0, 0],
    [2, 1, 2, 10, 0, 0],
    [2, 2, 0, 6, 6, 0],
    [2, 2, 0, 7, 7, 0],
    [2, 2, 0, 8, 8, 0],
    [2, 2, 0, 9, 9, 0],
    [2, 2, 0, 10, 0, 0],
    [3, 4, 0, 11, 11, 0],
    [3, 4, 0, 12, 0, 0],
    [2, 3, 0, 13, 0, 0]], np.int32)
HAND_XYZ = np.array([[0, 0, 0], [10, 0, 0], [0, 20, 0], [-10, 0, 0], [11, 0, 0], [1, 20, 0], [2, 20, 0], [3, 20, 0],
                     [4, 20, 0], [5, 20, 0], [12, 0, 0], [14, 0, 0], [-12, 0, 0]], np.float32)
# log-scales (all three axes): the root 2, row 2 1 (both above the volume 1), rows 1, 3, 4 -1 (below), leaves 0
HAND_SCALING = np.repeat(np.array([2, -1, 1, -1, -1, 0, 0, 0, 0, 0, 0, 0, 0], np.float32)[:, None], 3, axis=1)
HAND_ARGS = dict(root=0, volume=1.0, tg=0.5, min_size=3)


def hand():
    return HAND_NODES.copy(), HAND_XYZ.copy(), HAND_SCALING.copy()


def malformed():
    """name -> a 13-row table that breaks contract 1."""
    out = {}
    for name, (row, col, val) in dict(member_out_of_range=(2, 3, 99), member_is_the_root=(1, 3, 0),
                                      node_in_two_lists=(3, 3, 4), list_cycles_within_child_count=(6, 4, 5),
                                      negative_child_count=(4, 2, -1)).items():
        nd = HAND_NODES.copy()
        nd[row, col] = val
        out[name] = nd
    return out
