"""Two rasterizer settings that every other GPU test holds at one value: scale_modifier != 1, and an active SH
degree below the stored row count (training keeps 16 rows -- alt: dc + 15 -- while active_sh_degree climbs 0 -> 3).

Every path that reads the modifier (k_preprocess, k_preprocess_sh2, cov3d_exact and the cov3D backward of
k_gauss_bwd) and every SH specialisation (k_preprocess_sh2, k_sh_bwd, k_sh_bwd_jac2, k_sh_from_colour is in
test_gpu_dp.py) runs against the oracle under the unchanged gates: radii bit-exact, image L-inf <= 1e-4 with no
pixel over it, assert_grad on every gradient.  The oracle is pinned on both axes against float64 autograd by
tests/test_oracle.py::test_oracle_scale_modifier_and_partial_degree; dscale is the gradient of the effective scale
scale_modifier * scale (DESIGN A-23).  Each case prints its worst forward L-inf and grad_check ratio.

Measured on an MI355X (forward L-inf against the 1e-4 gate; worst grad_check ratio against 1, and its tensor):
  hot (P, rows-degree, D, mod)   2000,3,3,1.7: 1.8e-7, 0.026 dscale     2000,3,1,0.5: 6.0e-8, 0.010 dopacity
                                 1500,3,0,1.0: 1.2e-7, 0.017 dmean2D    1500,3,2,2.5: 1.8e-7, 0.061 dopacity
                                 1500,2,1,1.0: 1.8e-7, 0.031 dmean3D     800,1,0,1.3: 1.5e-7, 0.035 dmean3D
  cov3D_precomp mod 3: 1.2e-7, 0.015          colors_precomp mod 1.7: 1.8e-7, 0.011
  in-kernel hierarchy (D, mod)   3,1.7: 1.8e-7, 0.008 dmean2D; with roots 0.017 drot
                                 1,1.0: 1.8e-7, 0.006 dmean2D; with roots 0.008 dmean3D
  interpolation weights D 2, mod 0.6: 1.2e-7, 0.011 dscale
  alt (P, rows-degree, D, aa, mod)  2000,3,1,T,1.7: 1.8e-7, 0.086 dopacity   1500,3,0,F,0.5: 1.2e-7, 0.010 dopacity
                                    1500,3,2,T,1.0: 1.2e-7, 0.032 dmean2D    1200,2,1,F,2.5: 1.8e-7, 0.314 dopacity
  generic binning 20000, D 1, mod 1.7: 1.2e-7, 0.016 dmean2D; 0.66 s, test_generic_binning_path_backward 0.78 s
The bit-exact cases (lists, pre-scaled scales, cov3D_precomp at 3 against 1, debug=True) hold with no fallback.
"""
import numpy as np
import pytest
import torch

from hlgs_core import synthetic as S
from oracle import oracle as O
from helpers import (assert_grad, binned, drops_empty, gpu_render, grad_check, image_check, oracle_render,
                     settings_for)
from test_gpu_alt import _alt_scene

pytestmark = pytest.mark.gpu
DEV = "cuda"
FWD_TOL = 1e-4
GRADS = ("dmean3D", "dmean2D", "dopacity", "dscale", "drot", "dsh", "ddc")


def _leaves(sc, alt):
    """The scene's parameters as leaf tensors, kept across several renders (see _render)."""
    names = ("means3D", "opacities", "scales", "rotations", "shs") + (("dc",) if alt else ())
    return {k: torch.tensor(np.ascontiguousarray(sc[k]), device=DEV, requires_grad=True) for k in names}


def _render(p, cam, D, mod, g, alt=False, aa=True, debug=False, hier=None):
    """One forward + backward through the public API on the leaves p, whose .grad is dropped first: the gradient
    buffers of this call are new allocations (what the allocator hands back from the last call's, not zeros).
    Gradients come back under the oracle's names."""
    for v in p.values():
        v.grad = None
    m2 = torch.zeros_like(p["means3D"], requires_grad=True)
    if alt:
        from alt_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
        rast = GaussianRasterizer(GaussianRasterizationSettings(
            image_height=cam["H"], image_width=cam["W"], tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"],
            bg=cam["bg"].to(DEV), scale_modifier=mod, viewmatrix=cam["viewmatrix"].to(DEV),
            projmatrix=cam["projmatrix"].to(DEV), sh_degree=D, campos=cam["campos"].to(DEV), prefiltered=False,
            debug=debug, antialiasing=aa))
        color, radii, invd = rast(means3D=p["means3D"], means2D=m2, opacities=p["opacities"], dc=p["dc"],
                                  shs=p["shs"], scales=p["scales"], rotations=p["rotations"])
    else:
        from diff_gaussian_rasterization import GaussianRasterizer
        rast = GaussianRasterizer(settings_for(cam, D, DEV, debug=debug, hierarchy=hier, scale_modifier=mod))
        color, radii, invd = rast(means3D=p["means3D"], means2D=m2, opacities=p["opacities"], shs=p["shs"],
                                  scales=p["scales"], rotations=p["rotations"])
    torch.autograd.backward([color, invd], [torch.tensor(g[0], device=DEV), torch.tensor(g[1], device=DEV)])
    n = lambda t: t.detach().cpu().numpy()  # noqa: E731
    out = dict(color=n(color), radii=n(radii), invdepth=n(invd), dmean3D=n(p["means3D"].grad), dmean2D=n(m2.grad),
               dopacity=n(p["opacities"].grad), dscale=n(p["scales"].grad), drot=n(p["rotations"].grad),
               dsh=n(p["shs"].grad))
    if alt:
        out["ddc"] = n(p["dc"].grad)
    return out


def _reference(sc, cam, D, mod, g, drop_empty=False):
    """The oracle on the same scene with the same two settings."""
    scene = dict(sc, sh_degree=D, scale_modifier=mod)
    fr = O.forward(scene, S.cam_numpy(cam), drop_empty=drop_empty)
    gr = O.backward(fr, scene, *g)
    out = dict(color=fr.color, radii=fr.radii, invdepth=fr.invdepth, frame=fr)
    out.update({k: gr[k] for k in GRADS if k != "ddc" or sc.get("alt")})
    return out


def _check(tag, gpu, ref):
    """The suite's gates, unchanged; prints the case's worst forward L-inf and grad_check ratio before asserting."""
    keys = [k for k in GRADS if k in ref]
    fwd = {k: image_check(gpu[k], ref[k], FWD_TOL) for k in ("color", "invdepth")}
    ratios = {k: grad_check(gpu[k][..., :ref[k].shape[-1]], ref[k])[0] for k in keys}
    worst = max(ratios, key=ratios.get)
    print(f"\n[settings] {tag}: forward L-inf {max(v[0] for v in fwd.values()):.3e}, "
          f"worst grad_check ratio {ratios[worst]:.4f} ({worst})")
    np.testing.assert_array_equal(gpu["radii"], ref["radii"])
    for k, (mx, nbad, ok) in fwd.items():
        assert ok, f"{k} L-inf {mx} ({nbad} pixels over {FWD_TOL})"
    for k in keys:
        assert_grad(k, gpu[k][..., :ref[k].shape[-1]], ref[k])


def _active_rows(D, alt):
    """Rows of `shs` the active degree reads (alt: the rest rows, dc apart)."""
    return (D + 1) ** 2 - (1 if alt else 0)


def _prefill(p, cam, rows_deg, D, mod, g, signal=True, **kw):
    """Before a case with D below the stored degree: a backward at the full degree on the same leaves, then a NaN
    tensor of the SH gradient's size, allocated and freed.  The backward writes every row without a memset, into
    buffers the allocator hands it from those freed blocks: a row it left out would show the old values, not a fresh
    allocation's zeros.  signal=False: the full-degree gradient is zero too (see _hierarchy_case)."""
    if D == rows_deg:
        return
    pre = _render(p, cam, rows_deg, mod, g, **kw)
    if signal:
        assert np.abs(pre["dsh"][:, _active_rows(D, kw.get("alt", False)):]).max() > 0
    for v in p.values():
        v.grad = None
    stale = torch.full_like(p["shs"], float("nan"))
    del stale


def _assert_inactive_rows_zero(gpu, ref, D, alt, signal=True):
    a = _active_rows(D, alt)
    assert np.all(ref["dsh"][:, a:] == 0)
    assert np.all(gpu["dsh"][:, a:] == 0), f"inactive SH rows (from row {a}) hold non-zero gradient"
    if a and signal:
        assert np.abs(gpu["dsh"][:, :a]).max() > 0


# a. the hot path: k_preprocess_sh2<false, 3M> + k_sh_bwd_jac2<M> ------------------------------------------------------

HOT = [(2000, 3, 3, 128, 96, 1.7), (2000, 3, 1, 128, 96, 0.5), (1500, 3, 0, 100, 75, 1.0), (1500, 3, 2, 100, 75, 2.5),
       (1500, 2, 1, 96, 80, 1.0), (800, 1, 0, 80, 64, 1.3)]


@pytest.mark.parametrize("P,rows_deg,D,W,H,mod", HOT)
def test_hot_path_modifier_and_partial_degree(P, rows_deg, D, W, H, mod):
    cam = S.make_camera(W, H)
    sc = S.make_gaussians(P, rows_deg, cam, seed=P + D)
    g = S.upstream_grads(W, H, seed=1)
    p = _leaves(sc, False)
    _prefill(p, cam, rows_deg, D, mod, g)
    gpu = _render(p, cam, D, mod, g)
    ref = _reference(sc, cam, D, mod, g)
    _check(f"hot P={P} rows={rows_deg} D={D} mod={mod}", gpu, ref)
    _assert_inactive_rows_zero(gpu, ref, D, False)


# b. tile lists: rects (and alt's per-tile culling) depend on the conic, hence on the modifier --------------------------

def test_lists_bit_exact_with_modifier():
    from diff_gaussian_rasterization import _C
    P, W, H, mod = 2000, 128, 96, 1.7
    cam = S.make_camera(W, H)
    sc = S.make_gaussians(P, 3, cam, seed=P + 3)
    fr = O.forward(dict(sc, scale_modifier=mod), S.cam_numpy(cam), drop_empty=drops_empty(P))
    fr1 = O.forward(dict(sc), S.cam_numpy(cam), drop_empty=drops_empty(P))
    assert fr.R > fr1.R  # the modifier changes the lists
    t = lambda a: torch.tensor(a, device=DEV)  # noqa: E731
    e = torch.empty(0, device=DEV)
    out = _C.rasterize_gaussians(cam["bg"], e, e, e, e, t(sc["means3D"]), e, t(sc["opacities"]), t(sc["scales"]),
                                 t(sc["rotations"]), mod, e, cam["viewmatrix"], cam["projmatrix"], cam["tanfovx"],
                                 cam["tanfovy"], H, W, t(sc["shs"]), 3, cam["campos"], False, False, True)
    assert out[0] == fr.R
    kept = binned(fr)
    np.testing.assert_array_equal(_C.inspect_ranges(out[5], W, H).cpu().numpy().astype(np.uint32), fr.ranges)
    np.testing.assert_array_equal(_C.inspect_point_list(out[4], kept, P).cpu().numpy().astype(np.uint32),
                                  fr.point_list[:kept])
    N = W * H
    n_contrib = _C._field(out[5], (4 * N + 255) // 256 * 256, N, torch.int32).cpu().numpy()
    np.testing.assert_array_equal(n_contrib, fr.n_contrib.astype(np.int32))
    np.testing.assert_array_equal(out[7].cpu().numpy(), fr.seen)


def test_alt_lists_bit_exact_with_modifier():
    from alt_gaussian_rasterization import _C
    from diff_gaussian_rasterization import _C as HC
    P, W, H, mod, D = 2000, 128, 96, 1.7, 1
    sc, cam = _alt_scene(P, 3, W, H, seed=P + 1)
    fr = O.forward(dict(sc, sh_degree=D, scale_modifier=mod), S.cam_numpy(cam), drop_empty=drops_empty(P))
    fr1 = O.forward(dict(sc, sh_degree=D), S.cam_numpy(cam), drop_empty=drops_empty(P))
    assert fr.R > fr1.R
    t = lambda a: torch.tensor(a, device=DEV)  # noqa: E731
    e = torch.empty(0, device=DEV)
    out = _C.rasterize_gaussians(cam["bg"], t(sc["means3D"]), e, t(sc["opacities"]), t(sc["scales"]),
                                 t(sc["rotations"]), mod, e, cam["viewmatrix"], cam["projmatrix"], cam["tanfovx"],
                                 cam["tanfovy"], H, W, t(sc["dc"]), t(sc["shs"]), D, cam["campos"], False, True, False)
    num_rendered, _, color, _, radii, _, binning, img, _ = out
    assert num_rendered == fr.R
    np.testing.assert_array_equal(radii.cpu().numpy(), fr.radii)
    np.testing.assert_array_equal(HC.inspect_ranges(img, W, H).cpu().numpy().astype(np.uint32), fr.ranges)
    kept = binned(fr)
    np.testing.assert_array_equal(HC.inspect_point_list(binning, kept, P).cpu().numpy().astype(np.uint32),
                                  fr.point_list[:kept])
    N = W * H
    n_contrib = HC._field(img, (4 * N + 255) // 256 * 256, N, torch.int32).cpu().numpy()
    np.testing.assert_array_equal(n_contrib, fr.n_contrib.astype(np.int32))
    mx, nbad, ok = image_check(color.cpu().numpy(), fr.color, FWD_TOL)
    assert ok, (mx, nbad)


# c. modifier m == scales pre-multiplied by float32(m), without the oracle ---------------------------------------------

@pytest.mark.parametrize("alt", [False, True])
@pytest.mark.parametrize("m", [0.5, 1.7])
def test_modifier_equals_prescaled_scales(alt, m):
    """A render at scale_modifier = m against the same scene with scales = float32(m) * scales at modifier 1.
    mod * scale is the first operation on the scale in cov3d_fwd, cov3d_exact and the cov3D backward, and
    1.0f * x == x, so both runs do the same float operations: radii, colour, inverse depth and every gradient are
    bit-identical.  That includes dscale, which the backward neither divides nor multiplies by m (DESIGN A-23)."""
    P, W, H = 2000, 128, 96
    if alt:
        sc, cam = _alt_scene(P, 3, W, H, seed=61, aa=True)
    else:
        cam = S.make_camera(W, H)
        sc = S.make_gaussians(P, 3, cam, seed=60)
    pre = dict(sc, scales=np.ascontiguousarray(np.float32(m) * sc["scales"]))
    assert pre["scales"].dtype == np.float32
    g = S.upstream_grads(W, H, seed=1)
    a = _render(_leaves(sc, alt), cam, 3, m, g, alt=alt)
    b = _render(_leaves(pre, alt), cam, 3, 1.0, g, alt=alt)
    assert (a["radii"] > 0).sum() > P // 4 and np.abs(a["dscale"]).max() > 0
    for k in a:
        np.testing.assert_array_equal(a[k].view(np.uint32) if a[k].dtype == np.float32 else a[k],
                                      b[k].view(np.uint32) if b[k].dtype == np.float32 else b[k], err_msg=k)


# d. paths where the modifier is inert, or is the only reader ----------------------------------------------------------

def test_cov3d_precomp_ignores_modifier():
    """cov3D_precomp (built by the oracle at modifier 1): rendered at scale_modifier = 3 the frame and every gradient are
    bit-identical to the same call at 1, and match the oracle given the same setting."""
    cam = S.make_camera(80, 64)
    sc = S.make_gaussians(800, 1, cam, seed=0)
    fr = O.forward(dict(means3D=sc["means3D"], opacities=sc["opacities"], shs=sc["shs"], sh_degree=1,
                        scales=sc["scales"], rotations=sc["rotations"]), S.cam_numpy(cam))
    sc["cov3D_precomp"] = fr.cov3D.copy()
    g = S.upstream_grads(80, 64, seed=1)
    one = gpu_render(sc, cam, grads=g, use_cov=True, scale_modifier=1.0)
    three = gpu_render(sc, cam, grads=g, use_cov=True, scale_modifier=3.0)
    for k in one:
        np.testing.assert_array_equal(one[k], three[k], err_msg=k)
    ref = oracle_render(sc, cam, grads=g, use_cov=True, scale_modifier=3.0)
    np.testing.assert_array_equal(three["radii"], ref["radii"])
    mx, nbad, ok = image_check(three["color"], ref["color"], FWD_TOL)
    assert ok, (mx, nbad)
    ratios = {k: grad_check(three[k][..., :ref[k].shape[-1]], ref[k])[0] for k in ref if k.startswith("d")}
    print(f"\n[settings] cov3D_precomp mod=3: forward L-inf {mx:.3e}, worst grad_check ratio {max(ratios.values()):.4f}")
    for k in ratios:
        assert_grad(k, three[k][..., :ref[k].shape[-1]], ref[k])


def test_colors_precomp_with_modifier():
    """colors_precomp: the generic k_preprocess<false, false> reads the modifier; d_scales / d_rotations from the
    cov3D backward."""
    cam = S.make_camera(80, 64)
    sc = S.make_gaussians(800, 0, cam, seed=0)
    sc["colors_precomp"] = np.random.default_rng(3).uniform(0, 1, (800, 3)).astype(np.float32)
    g = S.upstream_grads(80, 64, seed=1)
    gpu = gpu_render(sc, cam, grads=g, use_colors=True, scale_modifier=1.7)
    ref = oracle_render(sc, cam, grads=g, use_colors=True, scale_modifier=1.7, drop_empty=drops_empty(800))
    ref1 = oracle_render(sc, cam, use_colors=True)
    assert not np.array_equal(ref["radii"], ref1["radii"])
    np.testing.assert_array_equal(gpu["radii"], ref["radii"])
    fwd = [image_check(gpu[k], ref[k], FWD_TOL) for k in ("color", "invdepth")]
    ratios = {k: grad_check(gpu[k][..., :ref[k].shape[-1]], ref[k])[0] for k in ref if k.startswith("d")}
    print(f"\n[settings] colors_precomp mod=1.7: forward L-inf {max(f[0] for f in fwd):.3e}, "
          f"worst grad_check ratio {max(ratios.values()):.4f}")
    assert all(f[2] for f in fwd), fwd
    assert {"d_scales", "d_rotations", "d_colors_precomp"} <= set(ratios)
    for k in ratios:
        assert_grad(k, gpu[k][..., :ref[k].shape[-1]], ref[k])


# e. in-kernel hierarchy mode ------------------------------------------------------------------------------------------

def _hierarchy_case(tag, scene, cam, hier_np, D, mod, rows_deg=3):
    """scene: the oracle's scene (full parameter arrays plus its hierarchy keys); hier_np: the same hierarchy under the
    settings' names.  Both sides get the same modifier and degree.  The reference drops the opacity, scale, rotation
    and SH gradients of every selected node that has a parent (backward.cu:458-494): where all of them have one, dsh is
    zero throughout and the check is that every row is written."""
    signal = "parent_indices" not in hier_np or bool((hier_np["parent_indices"] == -1).any())
    g = S.upstream_grads(cam["W"], cam["H"])
    ref = _reference(scene, cam, D, mod, g)
    hier = {k: torch.tensor(v, device=DEV) for k, v in hier_np.items()}
    p = _leaves(scene, False)
    _prefill(p, cam, rows_deg, D, mod, g, signal=signal, hier=hier)
    gpu = _render(p, cam, D, mod, g, hier=hier)
    _check(tag, gpu, ref)
    _assert_inactive_rows_zero(gpu, ref, D, False, signal=signal)


@pytest.mark.parametrize("mod,D,roots", [(1.7, 3, False), (1.0, 1, False), (1.7, 3, True), (1.0, 1, True)])
def test_in_kernel_hierarchy_mode_modifier_and_partial_degree(mod, D, roots):
    """The setup of test_gpu_lod.py::test_in_kernel_hierarchy_mode_matches_oracle on 16 rows: k_preprocess<true, false>,
    k_gauss_bwd<true, .> and k_sh_bwd<true, 16, false>.  That cut selects no root, so every selected node's scale,
    rotation, opacity and SH gradients are dropped; roots=True renders every fourth selected node as a root
    (parent_indices -1: no lerp towards a parent, gradients kept), so the modifier in the cov3D backward and the active
    rows of the SH backward carry values in this mode too."""
    from test_gpu_lod import _tree
    h, _ = _tree(1500)
    cam = S.make_camera(128, 96)
    vp = cam["campos"].numpy()
    n, ri, pi, ni = O.expand_to_size_dynamic(h["nodes"], h["means3D"], h["scales"], 0.004, vp,
                                             np.array([0, 0, 1], np.float32))
    ts, kids = O.interp_weights_dynamic(ni[:n], 0.004, h["nodes"], h["means3D"], h["scales"], vp)
    root_rows = h["nodes"][ri[:n], 1] < 0
    if roots:
        root_rows[::4] = True
    pidx = np.where(root_rows, -1, pi[:n]).astype(np.int32)
    assert h["shs"].shape[1] == 16
    scene = dict(means3D=h["means3D"], opacities=h["opacities"], shs=h["shs"], scales=h["scales"],
                 rotations=h["rotations"], indices=ri[:n], parent_indices=pidx, ts=ts, kids=kids)
    hier = dict(render_indices=ri[:n], parent_indices=pidx, interpolation_weights=ts, num_node_kids=kids)
    _hierarchy_case(f"in-kernel hierarchy D={D} mod={mod} roots={roots}", scene, cam, hier, D, mod)


def test_interpolation_weights_modifier_and_partial_degree():
    """The setup of test_gpu_lod.py::test_interpolation_weights_without_render_indices at modifier 0.6 and degree 2 on
    16 rows: k_preprocess_sh2<., true>."""
    cam = S.make_camera(160, 112)
    sc = S.make_gaussians(3000, 3, cam, seed=5)
    rng = np.random.default_rng(11)
    ts = rng.uniform(0.05, 1.0, 3000).astype(np.float32)
    kids = rng.integers(1, 9, 3000).astype(np.int32)
    scene = dict(sc, ts=ts, kids=kids)
    _hierarchy_case("interpolation weights D=2 mod=0.6", scene, cam,
                    dict(interpolation_weights=ts, num_node_kids=kids), 2, 0.6)


# f. the alt rasterizer ------------------------------------------------------------------------------------------------

ALT = [(2000, 3, 1, 128, 96, True, 1.7, (0.0, 0.0, 0.0)), (1500, 3, 0, 100, 75, False, 0.5, (0.0, 0.0, 0.0)),
       (1500, 3, 2, 100, 75, True, 1.0, (0.0, 0.0, 0.0)), (1200, 2, 1, 96, 64, False, 2.5, (0.3, 0.6, 0.9))]


@pytest.mark.parametrize("P,rows_deg,D,W,H,aa,mod,bg", ALT)
def test_alt_modifier_and_partial_degree(P, rows_deg, D, W, H, aa, mod, bg):
    """D = 0 with the 15 rest rows present is not test_alt_degree0_without_rest_gives_dc_no_gradient's path (rows
    absent, SH backward skipped): here the SH backward runs, ddc is non-zero and every rest row is zero."""
    sc, cam = _alt_scene(P, rows_deg, W, H, seed=P + D, bg=bg, aa=aa)
    g = S.upstream_grads(W, H, seed=1)
    p = _leaves(sc, True)
    _prefill(p, cam, rows_deg, D, mod, g, alt=True, aa=aa)
    gpu = _render(p, cam, D, mod, g, alt=True, aa=aa)
    ref = _reference(sc, cam, D, mod, g)
    _check(f"alt P={P} rows={rows_deg} D={D} aa={aa} mod={mod}", gpu, ref)
    _assert_inactive_rows_zero(gpu, ref, D, True)
    assert np.abs(gpu["ddc"]).max() > 0 and np.abs(ref["ddc"]).max() > 0


# g. the generic binning path ------------------------------------------------------------------------------------------

def test_generic_binning_path_modifier_and_partial_degree():
    """2064 x 2048, the smallest grid above the LDS binning's 16,384 tiles (as
    test_gpu_lod.py::test_generic_binning_path_backward, with a third of its Gaussians): the generic k_preprocess with
    SH and the SH backward that reads the rows, at modifier 1.7 and degree 1 on 16 rows."""
    W, H, P, D, mod = 2064, 2048, 20_000, 1, 1.7
    cam = S.make_camera(W, H)
    sc = S.make_gaussians(P, 3, cam, seed=31)
    g = S.upstream_grads(W, H, seed=4)
    p = _leaves(sc, False)
    _prefill(p, cam, 3, D, mod, g)
    gpu = _render(p, cam, D, mod, g)
    ref = _reference(sc, cam, D, mod, g, drop_empty=drops_empty(P))
    _check(f"generic binning P={P} D={D} mod={mod}", gpu, ref)
    _assert_inactive_rows_zero(gpu, ref, D, False)


# i. debug=True: a synchronisation after every stage, nothing else -----------------------------------------------------

@pytest.mark.parametrize("alt", [False, True])
def test_debug_flag_changes_no_value(alt, tmp_path, monkeypatch):
    """debug=True makes the library synchronise after every stage (check_stage); colour, inverse depth, radii and every
    gradient stay bit-identical.  Run from a scratch directory: the alt wrapper writes its argument snapshot to the
    working directory if a call fails."""
    monkeypatch.chdir(tmp_path)
    P, W, H = 2000, 128, 96
    if alt:
        sc, cam = _alt_scene(P, 3, W, H, seed=71, bg=(0.1, 0.2, 0.3))
    else:
        cam = S.make_camera(W, H, bg=(0.1, 0.2, 0.3))
        sc = S.make_gaussians(P, 3, cam, seed=70)
    g = S.upstream_grads(W, H, seed=1)
    p = _leaves(sc, alt)
    plain = _render(p, cam, 3, 1.0, g, alt=alt)
    dbg = _render(p, cam, 3, 1.0, g, alt=alt, debug=True)
    assert (plain["radii"] > 0).sum() > P // 4
    for k in plain:
        np.testing.assert_array_equal(plain[k], dbg[k], err_msg=k)
    assert not list(tmp_path.iterdir())
