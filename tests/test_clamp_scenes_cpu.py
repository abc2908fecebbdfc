"""The scene builders of tests/clamp_scenes.py do what tests/test_gpu_clamps.py rests on, asserted from the oracle alone
(conditions on the inputs: where a seed misses one, the seed changes, not the threshold).  Every (P, W, H, seed) the
GPU tests use is listed in clamp_scenes.FRUSTUM_SIZES / AA_SIZES; they import the lists.

"Contributing" means dopacity != 0 under S.upstream_grads: the Gaussian reached a pixel at alpha >= 1/255 before the
pixel stopped, so its gradients are not trivially zero."""
import numpy as np
import pytest

import clamp_scenes as CS
from hlgs_core import synthetic as S
from oracle import oracle as O


def _frame(sc, cam):
    fr = O.forward(dict(sc), S.cam_numpy(cam))
    gr = O.backward(fr, dict(sc), *S.upstream_grads(cam["W"], cam["H"]))
    return fr, gr


def _aa_ratio(sc, cam):
    """det(cov) / det(cov + 0.3 I) of the EWA-projected covariance, float64, for a camera at the origin looking down
    +z and centres inside the frustum (aa_floor_scene)."""
    m = sc["means3D"].astype(np.float64)
    x, y, z = m[:, 0], m[:, 1], m[:, 2]
    fx, fy = cam["W"] / (2 * cam["tanfovx"]), cam["H"] / (2 * cam["tanfovy"])
    zero = np.zeros_like(z)
    J = np.stack([np.stack([fx / z, zero, -fx * x / z ** 2], -1), np.stack([zero, fy / z, -fy * y / z ** 2], -1)], -2)
    R = S._quat_to_mat(sc["rotations"].astype(np.float64))
    Sig = np.einsum("nij,nj,nkj->nik", R, sc["scales"].astype(np.float64) ** 2, R)
    cov = J @ Sig @ J.transpose(0, 2, 1)
    a, b, c = cov[:, 0, 0], cov[:, 0, 1], cov[:, 1, 1]
    return (a * c - b * b) / ((a + 0.3) * (c + 0.3) - b * b)


def _cam(realcam, W, H):
    return None if realcam is None else S.real_camera(S.load_real_cameras()[realcam], W=W, H=H)


@pytest.mark.parametrize("unnormalised", [False, True], ids=["unit_q", "raw_q"])
@pytest.mark.parametrize("realcam", [None, CS.REALCAM], ids=["synthetic_cam", "reference_cam"])
@pytest.mark.parametrize("P,W,H,seed", CS.FRUSTUM_SIZES)
def test_frustum_scene_clamps_contributing_gaussians(P, W, H, seed, realcam, unnormalised):
    sc, cam = CS.frustum_clamp_scene(P, 3, W, H, seed, cam=_cam(realcam, W, H), unnormalised=unnormalised)
    assert sc["means3D"].shape == (P, 3) and sc["shs"].shape == (P, 16, 3)
    if realcam is not None:
        assert not np.allclose(cam["R"], np.eye(3))
    xc, yc = CS.clamp_classes(sc, cam)
    # the classes are the builder's row ranges, a quarter each, and no centre sits near a limit (1.25 / 1.32 x tanfov)
    rows = np.arange(P)
    np.testing.assert_array_equal(xc, rows < P // 2)
    np.testing.assert_array_equal(yc, (rows >= P // 4) & (rows < 3 * P // 4))
    t = CS.camera_space(sc["means3D"], cam)
    for r, tan in ((np.abs(t[:, 0] / t[:, 2]), cam["tanfovx"]), (np.abs(t[:, 1] / t[:, 2]), cam["tanfovy"])):
        assert not np.any((r > 1.26 * tan) & (r < 1.31 * tan)) and r.max() < 1.91 * tan
    fr, gr = _frame(sc, cam)
    contrib = gr["dopacity"][:, 0] != 0
    n = int(contrib.sum())
    assert n >= 100
    for name, cls in (("x", xc & ~yc), ("y", yc & ~xc), ("both", xc & yc), ("neither", ~xc & ~yc)):
        k = int((cls & contrib).sum())
        assert k >= 0.15 * n, f"{name}-clamped: {k} of {n} contributing Gaussians"
    for c in range(3):
        k = int((((fr.clamped >> c) & 1) != 0)[contrib].sum())
        assert 0.15 * n <= k <= 0.6 * n, f"channel {c} clamped on {k} of {n} contributing Gaussians"
        # a clamped channel's colour is exactly 0 and its row of dL/dsh exactly 0
        on = ((fr.clamped >> c) & 1) != 0
        assert np.all(fr.rgb[on, c] == 0) and np.all(gr["dsh"][on][:, :, c] == 0)
        assert np.abs(gr["dsh"][~on & contrib][:, 0, c]).min() > 0
    if unnormalised:
        off = np.abs(np.linalg.norm(sc["rotations"], axis=1) - 1)
        assert np.median(off) > 0.1 and off.max() > 0.25


def test_two_views_of_the_frustum_scene_clamp_different_channels():
    """tests/test_gpu_dp.py's colour-factored cases render the frustum scene's SH from two cameras: some channels
    clamp in one view only (the direction-dependent rows decide), so the rebuild's per-view masks differ."""
    sc, cams = CS.two_view_scene("frustum")
    for D in (3, 1):
        a, b, seen = CS.clamp_bits_of_two_views(sc, cams, D)
        bits = lambda m: int(np.unpackbits(m[seen]).sum())  # noqa: E731
        assert bits(a ^ b) >= 5 and bits(a & b) >= 1000, (bits(a ^ b), bits(a & b))


@pytest.mark.parametrize("alt", [False, True], ids=["hierarchy", "alt"])
@pytest.mark.parametrize("P,W,H,seed", CS.AA_SIZES)
def test_aa_floor_scene_sits_on_the_floor(P, W, H, seed, alt):
    sc, cam = CS.aa_floor_scene(P, W, H, seed)
    if alt:
        sc = CS.alt_layout(sc, antialiasing=True)
    fr, gr = _frame(sc, cam)
    floor = np.arange(P) < P // 2
    contrib = gr["dopacity"][:, 0] != 0
    assert contrib[floor].all() and contrib.all()
    # det / det_h of the projected covariance J W Sigma W^T J^T (float64, from the scene), on the right side of 2.5e-5
    # with a margin float32 cannot cross
    ratio = _aa_ratio(sc, cam)
    assert np.all(ratio[floor] <= 0.9 * 2.5e-5) and np.all(ratio[~floor] >= 1.1 * 2.5e-5)
    # and what the oracle did with it: the record opacity of a floor row is sqrt(2.5e-5) x its opacity, that of
    # every other row larger; a floor row still passes alpha >= 1/255 at its own pixel
    o = sc["opacities"][:, 0]
    hs = fr.conic_opacity[:, 3].astype(np.float64) / o
    np.testing.assert_allclose(hs[floor], 0.005, rtol=1e-6)
    np.testing.assert_allclose(hs[~floor], np.sqrt(ratio[~floor]), rtol=1e-3)
    assert np.all(fr.conic_opacity[floor, 3] >= 1.05 / 255)
    # every splat owns a pixel: centres within 0.05 px of distinct pixel centres
    assert np.abs(fr.means2D - np.rint(fr.means2D)).max() <= 0.0501
    pix = np.rint(fr.means2D).astype(int)
    assert len({(a, b) for a, b in pix}) == P
