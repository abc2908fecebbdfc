"""The hierarchy creator on the GPU (csrc/hier_build.hip, hlgs_core/hierarchy.py) against the recursive numpy
restatement of tests/hier_build_ref.py.

Exact: the node table, the leaf -> input row assignment, the leaf rows' position, opacity and SH, and position and SH of
every node merged from two leaves (float32 in the reference's operation order on both sides).  Everything downstream
of an eigen-decomposition is compared with the float64 restatement as the yardstick: the GPU may be at most 4x as far
from it as the float32 restatement is on the same scene (another eigen-solver, another summation order), with a floor
of 4 float32 ulps of the largest yardstick value.  Rotations are compared through R diag(s^2) R^T only."""
import functools

import numpy as np
import pytest
import torch

import hier_build_ref as R
from hlgs_core import hierarchy as H

pytestmark = pytest.mark.gpu
DEV = "cuda"
S = H.LDS_CAP
EPS = R.EPS32

# every size at which the code takes another path: one leaf, the smallest trees, around a wave (64) and two, around the
# in-LDS cap S (one workgroup / one top level), two and four top levels with uneven halves, and a size near 20,000
SIZES = [1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 127, 129, S - 1, S, S + 1, 2 * S, 2 * S + 1, 4 * S + 3, 20011]
CASES = [("random", n, 48) for n in SIZES if n < 20000] + [("random", 20011, 3), ("random", 65, 3)] + \
        [(kind, n, 3) for kind in ("grid", "same", "plane", "far") for n in (7, 129, S + 1, 2 * S + 1)]
IDS = [f"{k}-{n}-sh{f}" for k, n, f in CASES]


def _gpu_build(sc):
    t = lambda k: torch.tensor(sc[k], device=DEV)  # noqa: E731
    out = H.build_dynamic_hierarchy(t("xyz"), t("shs"), t("opacity"), t("scales"), t("rotations"))
    return [o.cpu() for o in out]


@functools.lru_cache(maxsize=None)
def _case(kind, n, shf):
    """(scene, GPU rows as numpy, float32 restatement, float64 restatement), computed once per case."""
    sc = R.make_scene(kind, n, shf)
    pos, shs, alpha, log_scales, rot, nodes = _gpu_build(sc)
    gpu = dict(pos=pos.numpy(), shs=shs.reshape(2 * n - 1, -1).numpy(), alpha=alpha.numpy().reshape(-1),
               log_scales=log_scales.numpy(), rot=rot.numpy(), nodes=nodes.numpy())
    assert shs.shape == ((2 * n - 1, shf // 3, 3)) and alpha.shape == (2 * n - 1, 1) and nodes.dtype == torch.int32
    return sc, gpu, R.build_ref(sc, np.float32), R.build_ref(sc, np.float64)


def _merged_of_two_leaves(nodes):
    n = len(nodes)
    inner = np.where(nodes[:, R.CHILD_COUNT] == 2)[0]
    c0 = inner + 1
    c1 = nodes[c0, R.NEXT_SIBLING]
    return inner[(nodes[c0, R.CHILD_COUNT] == 0) & (nodes[np.minimum(c1, n - 1), R.CHILD_COUNT] == 0)]


@pytest.mark.parametrize("kind,n,shf", CASES, ids=IDS)
def test_tree_leaves_and_first_merges_are_exact(kind, n, shf):
    sc, gpu, r32, _ = _case(kind, n, shf)
    np.testing.assert_array_equal(gpu["nodes"], r32["nodes"])
    closed, leafpos = R.closed_form_nodes(n) if n <= 5000 else (None, None)
    if closed is not None:
        np.testing.assert_array_equal(gpu["nodes"][:, :5], closed[:, :5])
    leaf = np.where(gpu["nodes"][:, R.CHILD_COUNT] == 0)[0]
    src = gpu["nodes"][leaf, R.MAX_SIDE]
    np.testing.assert_array_equal(np.sort(src), np.arange(n))
    np.testing.assert_array_equal(gpu["pos"][leaf], sc["xyz"][src])
    np.testing.assert_array_equal(gpu["alpha"][leaf], sc["opacity"][src])
    np.testing.assert_array_equal(gpu["shs"][leaf], sc["shs"][src])
    first = _merged_of_two_leaves(gpu["nodes"])
    assert n < 2 or len(first) > 0
    np.testing.assert_array_equal(gpu["pos"][first], r32["pos"][first])
    np.testing.assert_array_equal(gpu["shs"][first], r32["shs"][first])


@pytest.mark.parametrize("kind,n,shf", CASES, ids=IDS)
def test_leaf_covariance_survives(kind, n, shf):
    """A leaf's rotation is normalised, re-expressed by the aligner (matrix -> signed permutation -> quaternion) and
    its scales are stored as logs.  Rebuilt in float64 from the stored row, the covariance differs from the input's
    (float64, from the float32 inputs) by at most (64 + 2 (max|ln s| + 1)) eps32 s_max^2 per entry: the stored rotation
    matrix is within 16 eps32 per entry of the input's (3 eps from the normalisation, 6 from the quaternion -> matrix
    products, 4 from the matrix -> quaternion step, rounded up), which enters an entry sum_k R_ik s_k^2 R_jk twice over
    at most sqrt(3) of column mass (2 * 16 * sqrt(3) < 64); exp(fl(log s))^2 is within 2 (|ln s| + 1) eps32 of s^2."""
    sc, gpu, _, _ = _case(kind, n, shf)
    leaf = np.where(gpu["nodes"][:, R.CHILD_COUNT] == 0)[0]
    src = gpu["nodes"][leaf, R.MAX_SIDE]
    got = R.rebuilt_cov(gpu["rot"][leaf], gpu["log_scales"][leaf])
    q = sc["rotations"][src].astype(np.float64)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    s = sc["scales"][src].astype(np.float64)
    want = R.rebuilt_cov(q, np.log(s))
    bound = (64 + 2 * (np.abs(np.log(s)).max(axis=1) + 1)) * EPS * s.max(axis=1) ** 2
    err = np.abs(got - want).max(axis=(1, 2))
    print(f"leaf covariance: worst error / bound = {(err / bound).max():.3f}")
    assert (err <= bound).all(), (err / bound).max()


def _distances(gpu, r32, r64, rows):
    out = {}
    cov = {k: R.rebuilt_cov(v["rot"][rows], v["log_scales"][rows])
           for k, v in (("gpu", gpu), ("r32", r32), ("r64", r64))}
    for name in ("pos", "cov", "alpha", "shs"):
        g, a, b = (cov["gpu"], cov["r32"], cov["r64"]) if name == "cov" else \
            (gpu[name][rows].astype(np.float64), r32[name][rows].astype(np.float64), r64[name][rows])
        out[name] = (float(np.abs(g - b).max()), float(np.abs(a - b).max()), float(np.abs(b).max()))
    return out


@pytest.mark.parametrize("kind,n,shf", [c for c in CASES if c[1] > 1], ids=[i for c, i in zip(CASES, IDS) if c[1] > 1])
def test_merged_rows_are_as_close_to_float64_as_the_float32_restatement(kind, n, shf):
    _, gpu, r32, r64 = _case(kind, n, shf)
    rows = np.where(gpu["nodes"][:, R.CHILD_COUNT] == 2)[0]
    assert np.isfinite(gpu["pos"]).all() and np.isfinite(gpu["log_scales"]).all() and np.isfinite(gpu["rot"]).all()
    for name, (d_gpu, d_32, mag) in _distances(gpu, r32, r64, rows).items():
        print(f"{name}: |gpu - f64| = {d_gpu:.3e}, |f32 - f64| = {d_32:.3e}, largest |f64| = {mag:.3e}")
        assert d_gpu <= max(4 * d_32, 4 * EPS * mag), (name, d_gpu, d_32, mag)


@pytest.mark.parametrize("kind,n,shf", [c for c in CASES if c[1] > 1], ids=[i for c, i in zip(CASES, IDS) if c[1] > 1])
def test_every_node_is_aligned_with_its_parent(kind, n, shf):
    """Of the 24 proper signed permutations of a stored node's axes none scores higher against the stored parent than
    the stored one.  Evaluated in float64 from the stored quaternions, with the slack of what the kernel could not
    see: its float32 score (9 products and sums, 18 eps32), the float32 matrices it scored (6 eps32 per entry, two
    matrices, 9 entries) and the matrix -> quaternion -> matrix round trip of the winner (16 eps32 per entry, 9
    entries): 256 eps32 in all, rounded up."""
    _, gpu, _, _ = _case(kind, n, shf)
    child = np.arange(1, 2 * n - 1)
    mats = R.matrix_from_quat(gpu["rot"].astype(np.float64).T).transpose(2, 0, 1)
    Rc, Rp = mats[child], mats[gpu["nodes"][child, R.PARENT]]
    # orthonormal, right-handed axes
    assert np.abs(np.einsum("nji,njk->nik", Rc, Rc) - np.eye(3)).max() <= 64 * EPS
    assert (np.linalg.det(Rc) > 0).all()
    stored = (Rc * Rp).sum(axis=(1, 2))
    cand = Rc[:, :, R.CAND_COLS] * R.CAND_SIGN[None, None]            # (n, 3, 48, 3): row, candidate, column
    proper = np.linalg.det(cand.transpose(0, 2, 1, 3)) > 0            # (n, 48)
    score = np.einsum("nrcw,nrw->nc", cand, Rp)
    best = np.where(proper, score, -np.inf).max(axis=1)
    assert proper.sum(axis=1).tolist() == [24] * len(child)
    assert (best <= stored + 256 * EPS).all(), float((best - stored).max())


def test_two_runs_are_bitwise_equal():
    sc = R.make_scene("random", 4 * S + 3, 48, seed=3)
    a, b = _gpu_build(sc), _gpu_build(sc)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_links_hold():
    from mcmc_ref import check_links
    _, gpu, _, _ = _case("random", 4 * S + 3, 48)
    nodes = torch.tensor(gpu["nodes"])
    check_links(nodes, 0, nodes.shape[0])
    depth = gpu["nodes"][:, R.DEPTH]
    np.testing.assert_array_equal(depth[1:], depth[gpu["nodes"][1:, R.PARENT]] + 1)


def test_file_round_trip_is_byte_exact(tmp_path):
    import gaussian_hierarchy as GH
    sc = R.make_scene("random", 129, 48)
    out = _gpu_build(sc)
    path = tmp_path / "built.dhier"
    GH.write_dynamic_hierarchy(str(path), *out, 3)
    back = GH.load_dynamic_hierarchy(str(path))
    for x, y in zip(out, back):
        assert x.shape == y.shape and x.dtype == y.dtype
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_built_hierarchy_streams_and_renders():
    """assemble_hierarchy -> build_hierarchical_spt -> one SPTCache.step -> render, on a built hierarchy."""
    from tools_free_render import render_alt
    from hlgs_core import scene, spt
    from hlgs_core import synthetic as SY
    from hlgs_core.spt_cache import SPTCache
    cam = SY.make_camera(256, 192)
    g = SY.make_gaussians(4096, 3, cam, seed=8)
    t = lambda a: torch.tensor(a, device=DEV)  # noqa: E731
    out = [o.cpu() for o in H.build_dynamic_hierarchy(t(g["means3D"]), t(g["shs"]), t(g["opacities"]), t(g["scales"]),
                                                      t(g["rotations"]))]
    sky = dict(xyz=torch.tensor([[0.0, 0, 90], [0, 0, -90], [90, 0, 0], [-90, 0, 0]]),
               features_dc=torch.zeros(4, 1, 3), features_rest=torch.zeros(4, 3, 3),
               opacity_logits=torch.zeros(4, 1), scales=torch.zeros(4, 3), rotations=torch.eye(4)[:, :4])
    m = scene.assemble_hierarchy(*out, sky=sky)
    size, sky_n = m["nodes"].shape[0], m["skybox_points"]
    assert size == 4 + 2 * 4096 - 1 and sky_n == 4
    op = m["opacity"].clamp(0.01, 0.99)  # a merged opacity may exceed 1; the logit needs (0, 1)
    storage = dict(xyz=m["xyz"].contiguous(), f_dc=m["features_dc"].contiguous(),
                   f_rest=m["features_rest"].contiguous(), opacity=torch.log(op / (1 - op)),
                   scaling=m["scaling"].contiguous(), rotation=m["rotation"].contiguous())
    b = spt.build_hierarchical_spt(m["nodes"], storage["xyz"], storage["scaling"], sky_n, 3.0, 0.02, 20)
    cache = SPTCache(storage, b, sky_n)
    view = SY.make_camera(320, 240, T=np.array([0.04, 0.0, 0.3]))
    idx = cache.step(view["projmatrix"], view["campos"])
    assert idx.numel() > sky_n
    p = {k: storage[k][idx.long().cpu()].to(DEV).contiguous() for k in storage}
    img = render_alt(p, view, DEV)
    assert torch.isfinite(img).all() and float(img.max()) > 0


def test_mask_equals_the_restated_filter():
    sc = R.make_scene("random", 300, 48)
    sc["opacity"][1] = np.inf
    sc["opacity"][2] = np.nan
    sc["opacity"][3] = 0
    sc["opacity"][4] = -np.inf
    sc["scales"][5, 1] = 10.5
    sc["scales"][6, 2] = np.nan
    sc["rotations"][7, 3] = np.nan
    sc["xyz"][8, 1] = np.nan
    sc["shs"][9, 47] = np.nan
    sc["xyz"][10, 0] = np.inf     # kept by the creator
    sc["scales"][11, 0] = 10.0    # kept: the test is > 10
    sc["scales"][299, 0] = np.inf
    t = lambda k: torch.tensor(sc[k], device=DEV)  # noqa: E731
    mask = H.valid_gaussian_mask(t("xyz"), t("shs").reshape(300, 16, 3), t("opacity")[:, None], t("scales"),
                                 t("rotations"))
    assert mask.dtype == torch.bool and mask.is_cuda
    want = R.valid_mask_ref(sc)
    assert want.sum() == 300 - 10
    np.testing.assert_array_equal(mask.cpu().numpy(), want)


@pytest.mark.parametrize("field,value", [("opacity", 0.0), ("opacity", np.nan), ("xyz", np.inf), ("shs", np.nan),
                                         ("scales", np.inf), ("rotations", np.nan)])
def test_build_refuses_rows_it_cannot_merge(field, value):
    sc = R.make_scene("random", 2 * S + 1, 3)
    sc[field].reshape(2 * S + 1, -1)[S, 0] = value
    with pytest.raises(ValueError, match="non-finite value or has opacity 0"):
        _gpu_build(sc)


def test_build_refuses_an_empty_set():
    e = lambda *s: torch.zeros(s, device=DEV)  # noqa: E731
    with pytest.raises(ValueError, match="N = 0"):
        H.build_dynamic_hierarchy(e(0, 3), e(0, 16, 3), e(0, 1), e(0, 3), e(0, 4))
