"""Both rasterizers where the frustum clamp of the EWA Jacobian, the SH colour clamp at 0 and the anti-aliasing floor
fire, against the oracle (which tests/test_oracle.py pins against float64 autograd on the same kinds of scene).

hlgs_core.synthetic.make_gaussians reaches none of the three: its centres stay inside 1.1x the frustum (the clamp
starts at 1.3x), a colour channel goes negative about 2e-4 of the time, and its smallest splat is 0.3 px (the floor
needs ~0.04 px).  The scenes are tests/clamp_scenes.py's; tests/test_clamp_scenes_cpu.py asserts from the oracle that
they hold what they claim at every size used here.

Criteria are those of every other parity test, unchanged: radii equal, per-pixel L-inf <= 1e-4 with no exception,
every gradient within 1e-3 per tensor and element-wise (helpers.assert_grad).  On top, so that a fault in a clamped
row cannot hide behind larger unclamped ones: rel_err <= 1e-3 of dmean3D over the clamped contributing rows alone, and
of the SH gradient over the rows with a clamped channel, whose clamped channels are exactly 0."""
import numpy as np
import pytest
import torch

import clamp_scenes as CS
from hlgs_core import synthetic as S
from helpers import assert_grad, gpu_render, image_check, oracle_render, rel_err, settings_for
from oracle import oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
FWD_TOL = 1e-4
F0, F1, F2, F3 = CS.FRUSTUM_SIZES
A0, A1, A2 = CS.AA_SIZES


def _cam(realcam, W, H, bg=(0.0, 0.0, 0.0)):
    if realcam is None:
        return S.make_camera(W, H, bg=bg)
    return S.real_camera(S.load_real_cameras()[realcam], W=W, H=H, bg=bg)


def _frustum(size, deg, realcam=None, bg=(0.0, 0.0, 0.0), unnormalised=False):
    P, W, H, seed = size
    return CS.frustum_clamp_scene(P, deg, W, H, seed, cam=_cam(realcam, W, H, bg), unnormalised=unnormalised)


def _check_frame(gpu, ref, do_depth=True):
    np.testing.assert_array_equal(gpu["radii"], ref["radii"])
    for k in ("color", "invdepth") if do_depth else ("color",):
        mx, nbad, ok = image_check(gpu[k], ref[k], FWD_TOL)
        assert ok, f"{k}: L-inf {mx}, {nbad} pixels over {FWD_TOL}"
    for k in ref:
        if k.startswith("d"):
            assert_grad(k, gpu[k][..., :ref[k].shape[-1]], ref[k])


def _check_clamped_rows(gpu, ref, sc, cam, sh_keys=("d_shs",)):
    """The subsets: dmean3D over the contributing rows of each clamp class, the SH gradients over the rows with a
    clamped channel; the clamped channels' entries exactly 0, on both sides."""
    contrib = ref["dopacity"][:, 0] != 0
    xc, yc = CS.clamp_classes(sc, cam)
    for name, rows in (("x", xc & ~yc & contrib), ("y", yc & ~xc & contrib), ("both", xc & yc & contrib)):
        assert rows.sum() >= 10, (name, rows.sum())
        e = rel_err(gpu["dmean3D"][rows], ref["dmean3D"][rows])
        assert e <= 1e-3, f"dmean3D over the {rows.sum()} {name}-clamped contributing rows: rel err {e}"
    if not sh_keys:
        return
    bits = ref["frame"].clamped
    rows = (bits != 0) & contrib
    assert rows.sum() >= 30
    for k in sh_keys:
        if k not in ref or ref[k].shape[1] == 0:
            continue
        e = rel_err(gpu[k][rows], ref[k][rows])
        assert e <= 1e-3, f"{k} over the {rows.sum()} rows with a clamped channel: rel err {e}"
        for c in range(3):
            on = ((bits >> c) & 1) != 0
            assert on[contrib].sum() >= 10
            assert np.all(gpu[k][on][:, :, c] == 0) and np.all(ref[k][on][:, :, c] == 0), f"{k} channel {c}"


# ---- hierarchy rasterizer, frustum scene

@pytest.mark.parametrize("size,deg,do_depth,realcam", [(F0, 0, True, None), (F0, 3, False, CS.REALCAM),
                                                       (F1, 1, False, None), (F1, 2, True, CS.REALCAM),
                                                       (F2, 2, False, CS.REALCAM), (F3, 3, True, None)],
                         ids=["300-deg0-depth", "300-deg3-reference_cam", "1200-deg1", "1200-deg2-depth-reference_cam",
                              "2000-deg2-reference_cam", "3000-deg3-depth"])
def test_frustum_clamp_parity(size, deg, do_depth, realcam):
    """Contributing Gaussians outside 1.3x the frustum on one axis, the other, or both: the clamped t enters the
    Jacobian, dL/dt.x / dL/dt.y are cut, and dL/dt.z takes the clamped t (gauss_bwd.hip, backward.cu:185-186, 310-312).
    100 x 75 is no multiple of the 16-pixel tile; 2,000 and 3,000 Gaussians bin in more than one block."""
    sc, cam = _frustum(size, deg, realcam, bg=(0.2, 0.4, 0.6) if deg % 2 else (0.0, 0.0, 0.0))
    g = S.upstream_grads(cam["W"], cam["H"], seed=1, depth=do_depth)
    gpu = gpu_render(sc, cam, do_depth=do_depth, grads=g)
    ref = oracle_render(sc, cam, do_depth=do_depth, grads=g)
    _check_frame(gpu, ref, do_depth)
    _check_clamped_rows(gpu, ref, sc, cam)


@pytest.mark.parametrize("size,realcam", [(F0, None), (F2, CS.REALCAM)], ids=["300", "2000-reference_cam"])
def test_frustum_clamp_cov3d_precomp(size, realcam):
    """cov3D_precomp (the oracle's own fr.cov3D): the backward's dL/dcov3D output under the clamped Jacobian."""
    sc, cam = _frustum(size, 1, realcam)
    sc["cov3D_precomp"] = oracle_render(sc, cam)["frame"].cov3D.copy()
    g = S.upstream_grads(cam["W"], cam["H"], seed=1)
    gpu = gpu_render(sc, cam, grads=g, use_cov=True)
    ref = oracle_render(sc, cam, grads=g, use_cov=True)
    assert np.abs(ref["d_cov3D_precomp"]).max() > 0
    _check_frame(gpu, ref)
    _check_clamped_rows(gpu, ref, sc, cam)
    contrib = ref["dopacity"][:, 0] != 0
    xc, yc = CS.clamp_classes(sc, cam)
    rows = (xc | yc) & contrib
    e = rel_err(gpu["d_cov3D_precomp"][rows], ref["d_cov3D_precomp"][rows])
    assert e <= 1e-3, f"d_cov3D_precomp over the clamped contributing rows: rel err {e}"


def test_frustum_clamp_colors_precomp():
    sc, cam = _frustum(F1, 0, CS.REALCAM, bg=(0.3, 0.6, 0.9))
    sc["colors_precomp"] = np.random.default_rng(3).uniform(0, 1, (F1[0], 3)).astype(np.float32)
    g = S.upstream_grads(cam["W"], cam["H"], seed=1)
    gpu = gpu_render(sc, cam, grads=g, use_colors=True)
    ref = oracle_render(sc, cam, grads=g, use_colors=True)
    _check_frame(gpu, ref)
    _check_clamped_rows(gpu, ref, sc, cam, sh_keys=())


def test_frustum_clamp_scale_modifier():
    sc, cam = _frustum(F1, 2)
    g = S.upstream_grads(cam["W"], cam["H"], seed=1)
    gpu = gpu_render(sc, cam, grads=g, scale_modifier=1.7)
    ref = oracle_render(sc, cam, grads=g, scale_modifier=1.7)
    _check_frame(gpu, ref)
    _check_clamped_rows(gpu, ref, sc, cam)


# ---- tile lists and splat records, bit for bit

@pytest.mark.parametrize("size,deg,realcam", [(F0, 3, None), (F1, 0, CS.REALCAM), (F3, 2, CS.REALCAM)],
                         ids=["300", "1200-reference_cam", "3000-reference_cam"])
def test_frustum_clamp_lists_and_records_bit_exact(size, deg, realcam):
    """Off-screen centres with a conic from the clamped Jacobian: the footprint quadrant masks and the band test decide
    the tile lists from outside the frame.  point_list, ranges, n_contrib, seen and the splat records against the
    oracle run with the same drop_empty."""
    from test_gpu_realcam import _check_lists_and_records
    sc, cam = _frustum(size, deg, realcam)
    fr = _check_lists_and_records(sc, cam, deg)
    xc, yc = CS.clamp_classes(sc, cam)
    assert ((fr.seen > 0) & (xc | yc)).sum() >= 50  # clamped Gaussians reach pixels


@pytest.mark.parametrize("size,realcam", [(F1, None), (F3, CS.REALCAM)], ids=["1200", "3000-reference_cam"])
def test_frustum_clamp_alt_tile_culling_lists_bit_exact(size, realcam):
    """As test_gpu_alt.test_alt_tile_culling_lists_bit_exact: the alt rasterizer's exact per-tile culling of the
    off-screen splats' rects."""
    from alt_gaussian_rasterization import _C
    from diff_gaussian_rasterization import _C as HC
    from helpers import drops_empty
    sc, cam = _frustum(size, 1, realcam)
    sc = CS.alt_layout(sc)
    W, H = cam["W"], cam["H"]
    fr = O.forward(dict(sc), S.cam_numpy(cam), drop_empty=drops_empty(sc["means3D"].shape[0]))
    t = lambda a: torch.tensor(a, device=DEV)  # noqa: E731
    e = torch.empty(0, device=DEV)
    out = _C.rasterize_gaussians(cam["bg"], t(sc["means3D"]), e, t(sc["opacities"]), t(sc["scales"]),
                                 t(sc["rotations"]), 1.0, e, cam["viewmatrix"], cam["projmatrix"], cam["tanfovx"],
                                 cam["tanfovy"], H, W, t(sc["dc"]), t(sc["shs"]), 1, cam["campos"], False, True, False)
    num_rendered, _, color, invd, radii, geom, binning, img, _ = out
    assert num_rendered == fr.R
    np.testing.assert_array_equal(radii.cpu().numpy(), fr.radii)
    np.testing.assert_array_equal(HC.inspect_ranges(img, W, H).cpu().numpy().astype(np.uint32), fr.ranges)
    kept = int((fr.ranges[:, 1] - fr.ranges[:, 0]).sum())
    assert 0 < kept < fr.R
    np.testing.assert_array_equal(HC.inspect_point_list(binning, kept).cpu().numpy().astype(np.uint32),
                                  fr.point_list[:kept])
    N = W * H
    n_contrib = HC._field(img, (4 * N + 255) // 256 * 256, N, torch.int32).cpu().numpy()
    np.testing.assert_array_equal(n_contrib, fr.n_contrib.astype(np.int32))
    assert np.abs(color.cpu().numpy() - fr.color).max() <= 1e-4


# ---- alt rasterizer

def _alt_compare(sc, cam):
    from test_gpu_alt import _compare
    return _compare(sc, cam)


@pytest.mark.parametrize("size,deg,aa,realcam", [(F0, 3, True, None), (F1, 1, False, CS.REALCAM),
                                                 (F2, 2, True, CS.REALCAM), (F3, 3, False, None)],
                         ids=["300-aa", "1200-noaa-reference_cam", "2000-aa-reference_cam", "3000-noaa"])
def test_alt_frustum_clamp_parity(size, deg, aa, realcam):
    """The alt rasterizer (dc / rest split, antialiasing on and off) on the frustum scene: the clamp bits gate dc and
    the rest rows alike."""
    sc, cam = _frustum(size, deg, realcam, bg=(0.1, 0.2, 0.3))
    sc = CS.alt_layout(sc, aa)
    gpu, ref = _alt_compare(sc, cam)
    _check_clamped_rows(gpu, ref, sc, cam, sh_keys=("ddc", "dshs"))


def _check_floor_rows(gpu, ref, P):
    """dopacity of the floor rows as its own subset (at the floor it is 0.005 x the blend's gradient, and the opacity
    term of the covariance gradient is cut), and the scale gradient there, which is then the conic's alone."""
    floor = np.arange(P) < P // 2
    assert np.all(ref["dopacity"][floor, 0] != 0)
    e = rel_err(gpu["dopacity"][floor], ref["dopacity"][floor])
    assert e <= 1e-3, f"dopacity over the floor rows: rel err {e}"
    k = "d_scales" if "d_scales" in ref else "dscale"
    e = rel_err(gpu[k][floor], ref[k][floor])
    assert e <= 1e-3, f"{k} over the floor rows: rel err {e}"


@pytest.mark.parametrize("size", [A0, A1, A2], ids=["300", "1500", "3000"])
def test_alt_aa_floor_parity(size):
    P, W, H, seed = size
    sc, cam = CS.aa_floor_scene(P, W, H, seed, deg=1)
    gpu, ref = _alt_compare(CS.alt_layout(sc, True), cam)
    _check_floor_rows(gpu, ref, P)


@pytest.mark.parametrize("size,deg", [(A0, 1), (A1, 3), (A2, 0)], ids=["300", "1500", "3000"])
def test_aa_floor_parity(size, deg):
    """Splats of 0.005-0.03 px: det / det_h <= 2.5e-5, the AA factor is its floor 0.005 and d_inside = 0
    (gauss_bwd.hip); the other half of the scene is just above the floor.  90 x 70 is no multiple of 16."""
    P, W, H, seed = size
    sc, cam = CS.aa_floor_scene(P, W, H, seed, deg=deg)
    g = S.upstream_grads(W, H, seed=1)
    gpu = gpu_render(sc, cam, grads=g)
    ref = oracle_render(sc, cam, grads=g)
    _check_frame(gpu, ref)
    _check_floor_rows(gpu, ref, P)


# ---- quaternions used as given

@pytest.mark.parametrize("kind,size,realcam", [("frustum", F1, CS.REALCAM), ("plain", (1500, 100, 75, 6), None)],
                         ids=["frustum", "make_gaussians"])
def test_unnormalised_quaternions(kind, size, realcam):
    """cov3d_fwd and the cov3D backward take the quaternion as given (forward.cu:181-215, backward.cu:330-393):
    quaternions of norm 0.7-1.4, where R(q) is no rotation and dL/dq has a radial part."""
    P, W, H, seed = size
    if kind == "frustum":
        sc, cam = _frustum(size, 2, realcam, unnormalised=True)
    else:
        cam = _cam(realcam, W, H)
        sc = CS.unnormalise_quaternions(S.make_gaussians(P, 2, cam, seed=seed), seed)
    g = S.upstream_grads(W, H, seed=1)
    gpu = gpu_render(sc, cam, grads=g)
    ref = oracle_render(sc, cam, grads=g)
    _check_frame(gpu, ref)
    if kind == "frustum":
        _check_clamped_rows(gpu, ref, sc, cam)
    # the radial part of dL/dq, which a unit quaternion's gradient does not have under a normalising caller
    q = sc["rotations"].astype(np.float64)
    radial = (ref["d_rotations"] * q).sum(1)
    assert np.abs(radial).max() > 1e-3 * np.abs(ref["d_rotations"]).max()
    assert rel_err((gpu["d_rotations"] * q).sum(1), radial) <= 1e-3


# ---- hierarchy mode inside the kernel (the HIER instantiations)

def _hier_gpu(h, cam, deg, hier, g, gd):
    from diff_gaussian_rasterization import GaussianRasterizer
    t = lambda a, rg=False: torch.tensor(a, device=DEV, requires_grad=rg)  # noqa: E731
    rast = GaussianRasterizer(settings_for(cam, deg, DEV, hierarchy={k: t(v) for k, v in hier.items()}))
    m, o, sh, s, r = (t(h[k], True) for k in ("means3D", "opacities", "shs", "scales", "rotations"))
    m2 = torch.zeros_like(m, requires_grad=True)
    color, radii, invd = rast(means3D=m, means2D=m2, opacities=o, shs=sh, scales=s, rotations=r)
    ((color * t(g)).sum() + (invd * t(gd)).sum()).backward()
    out = dict(color=color.detach().cpu().numpy(), invdepth=invd.detach().cpu().numpy(), radii=radii.cpu().numpy())
    for name, leaf in (("dmean3D", m), ("dopacity", o), ("dscale", s), ("drot", r), ("dsh", sh), ("dmean2D", m2)):
        out[name] = leaf.grad.cpu().numpy()
    return out


def _check_hier(gpu, fr, gr):
    np.testing.assert_array_equal(gpu["radii"], fr.radii)
    for k, want in (("color", fr.color), ("invdepth", fr.invdepth)):
        mx, nbad, ok = image_check(gpu[k], want, FWD_TOL)
        assert ok, f"{k}: L-inf {mx}, {nbad} pixels over {FWD_TOL}"
    for name in ("dmean3D", "dopacity", "dscale", "drot", "dsh", "dmean2D"):
        assert_grad(name, gpu[name], gr[name])


def test_frustum_clamp_in_kernel_hierarchy_mode():
    """make_dynamic_hierarchy over the frustum scene's leaves, a cut and its weights from the oracle, rendered with the
    in-kernel lerp (as test_gpu_lod.test_in_kernel_hierarchy_mode_matches_oracle).  A selected node with a parent hands
    (1 - t) of its mean gradient to the parent and keeps none (backward.cu:458-494), so the clamped subset is taken
    over the parents all of whose selected children lie, with the parent, beyond the same frustum limit (the lerped
    centre then does too)."""
    P, W, H, seed = F1
    leaves, cam = CS.frustum_clamp_scene(P, 3, W, H, seed)
    h = S.make_dynamic_hierarchy(leaves)
    tau = 0.2  # the splats are wide (sigma / depth ~ 0.1-0.25): this cut runs through the tree's middle
    vp = cam["campos"].numpy()
    n, ri, pi, ni = O.expand_to_size_dynamic(h["nodes"], h["means3D"], h["scales"], tau, vp,
                                             np.array([0, 0, 1], np.float32))
    ts, kids = O.interp_weights_dynamic(ni[:n], tau, h["nodes"], h["means3D"], h["scales"], vp)
    assert 300 < n < P and ((ts > 0) & (ts < 1)).sum() > 100
    roots = h["nodes"][ri[:n], 1] < 0
    pidx = np.where(roots, -1, pi[:n]).astype(np.int32)
    scene = dict(means3D=h["means3D"], opacities=h["opacities"], shs=h["shs"], scales=h["scales"],
                 rotations=h["rotations"], sh_degree=3, indices=ri[:n], parent_indices=pidx, ts=ts, kids=kids)
    fr = O.forward(scene, S.cam_numpy(cam))
    g, gd = S.upstream_grads(W, H)
    gr = O.backward(fr, scene, g, gd)
    gpu = _hier_gpu(h, cam, 3, dict(render_indices=ri[:n], parent_indices=pidx, interpolation_weights=ts,
                                   num_node_kids=kids), g, gd)
    _check_hier(gpu, fr, gr)
    xc, yc = CS.clamp_classes(h, cam)
    side_x, side_y = np.sign(h["means3D"][:, 0]), np.sign(h["means3D"][:, 1])
    sel, par = ri[:n], np.where(pidx < 0, ri[:n], pidx)
    same = (xc[sel] & xc[par] & (side_x[sel] == side_x[par])) | (yc[sel] & yc[par] & (side_y[sel] == side_y[par]))
    rows = np.setdiff1d(np.unique(par[same & (pidx >= 0)]), np.unique(par[~same]))
    rows = rows[np.abs(gr["dmean3D"][rows]).max(1) > 0]
    assert rows.size >= 20, rows.size
    e = rel_err(gpu["dmean3D"][rows], gr["dmean3D"][rows])
    assert e <= 1e-3, f"dmean3D over {rows.size} parents of clamped selected nodes: rel err {e}"


@pytest.mark.parametrize("size,deg", [(F0, 1), (F2, 3)], ids=["300", "2000"])
def test_frustum_clamp_interpolation_weights_without_render_indices(size, deg):
    """The ts / kids-only path (test_gpu_lod.test_interpolation_weights_without_render_indices) on the frustum scene."""
    sc, cam = _frustum(size, deg)
    P, W, H, _ = size
    rng = np.random.default_rng(11)
    ts = rng.uniform(0.05, 1.0, P).astype(np.float32)
    kids = rng.integers(1, 9, P).astype(np.int32)
    scene = dict(sc, ts=ts, kids=kids)
    fr = O.forward(scene, S.cam_numpy(cam))
    g, gd = S.upstream_grads(W, H)
    gr = O.backward(fr, scene, g, gd)
    gpu = _hier_gpu(sc, cam, deg, dict(interpolation_weights=ts, num_node_kids=kids), g, gd)
    _check_hier(gpu, fr, gr)
    ref = dict(dopacity=gr["dopacity"], dmean3D=gr["dmean3D"], d_shs=gr["dsh"], frame=fr)
    _check_clamped_rows(dict(dmean3D=gpu["dmean3D"], d_shs=gpu["dsh"]), ref, sc, cam)
