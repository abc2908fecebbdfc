"""`alt_gaussian_rasterization._C` on MI355X.

Same entry points, argument order and return tuples as the reference extension
(submodules/alt-rasterizer/ext.cpp:15-19: rasterize_gaussians, rasterize_gaussians_backward,
compute_relocation, mark_visible, adamUpdate; rasterize_points.cu:43-306).  The rasterizer runs in libhlgs.so
with variant = HLGS_VARIANT_ALT: SH split into dc + rest, optional antialiasing, eigen-radius tile rect with
exact per-tile culling, inverse depth always rendered, and the alt backward's gradient conventions.

`num_buckets` and `sampleBuffer` are the reference's per-32-splat backward state
(rasterizer_impl.cu:268-290); the MI355X backward replays tiles from the forward's per-pixel state instead
and needs none, so they are returned as 0 and an empty tensor (both are only handed back to backward).
"""
import torch

from hlgs_core import _lib as L
from hlgs_core import dp
from hlgs_core import raster
from hlgs_core.raster import compute_relocation, mark_visible  # noqa: F401  (rasterize_points.cu:234-253, 284-306)


def _raster_args(bg, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix,
                 projmatrix, tan_fovx, tan_fovy, H, W, dc, sh, degree, campos, prefiltered, antialiasing, debug):
    if means3D.ndimension() != 2 or means3D.size(1) != 3:
        raise RuntimeError("means3D must have dimensions (num_points, 3)")
    P = means3D.size(0)
    # rasterize_points.cu:97-101: M = sh.size(1) when sh is non-empty (the higher-order coefficients)
    M = sh.size(1) if (sh is not None and sh.size(0) != 0 and sh.dim() > 1) else 0
    a, keep = raster.raster_args(L.VARIANT_ALT, P, P, M, bg, means3D, colors, opacity, scales, rotations,
                                 scale_modifier, cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, H, W, sh,
                                 degree, campos, prefiltered, debug, antialiasing=antialiasing, dc=raster._opt(dc))
    return a, keep, P, M


_binning_hint = raster.binning_hints[L.VARIANT_ALT]


def rasterize_gaussians(background, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp,
                        viewmatrix, projmatrix, tan_fovx, tan_fovy, image_height, image_width, dc, sh, degree, campos,
                        prefiltered, antialiasing, debug):
    """-> (num_rendered, num_buckets, color (3,H,W), invdepth (1,H,W), radii (P,), geomBuffer, binningBuffer,
    imgBuffer, sampleBuffer)  (rasterize_points.cu:43-136)."""
    lib = L.load()
    H, W = int(image_height), int(image_width)
    dev = means3D.device
    u8 = dict(dtype=torch.uint8, device=dev)
    if means3D.size(0) == 0:  # rasterize_points.cu:88-90, 99: nothing is launched, the outputs stay 0
        f32 = dict(dtype=torch.float32, device=dev)
        return (0, 0, torch.zeros((3, H, W), **f32), torch.zeros((1, H, W), **f32),
                torch.zeros((0,), dtype=torch.int32, device=dev), torch.empty((0,), **u8), torch.empty((0,), **u8),
                torch.empty((0,), **u8), torch.empty((0,), **u8))
    a, keep, P, _ = _raster_args(background, means3D, colors, opacity, scales, rotations, scale_modifier,
                                 cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, H, W, dc, sh, degree,
                                 campos, prefiltered, antialiasing, debug)
    n, color, invdepth, radii, geom, binning, img, _ = raster.forward(lib, a, _binning_hint, P, H, W, dev, True, False)
    return (n, 0, color, invdepth, radii, geom, binning, img, torch.empty((0,), **u8))


def rasterize_gaussians_backward(background, means3D, radii, colors, opacities, scales, rotations, scale_modifier,
                                 cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, dL_dout_color, dc, sh,
                                 dL_dout_invdepth, degree, campos, geomBuffer, R, binningBuffer, imageBuffer, B,
                                 sampleBuffer, antialiasing, debug, *, need_cov3D=True):
    """-> (dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_ddc, dL_dsh, dL_dscales,
    dL_drotations)  (rasterize_points.cu:138-232).  need_cov3D=False (the autograd wrapper without cov3D_precomp)
    returns an empty dL_dcov3D and skips writing its rows."""
    lib = L.load()
    H, W = int(dL_dout_color.size(1)), int(dL_dout_color.size(2))
    P = means3D.size(0)
    M = sh.size(1) if (sh is not None and sh.size(0) != 0 and sh.dim() > 1) else 0
    # a colour-factored view-DP exchange takes dL/dRGB instead of the dc / SH gradients (hlgs_core.dp.colour_factor);
    # not with an empty sh, whose SH backward does not run at all (A-19)
    fac = dp.colour_factor(sh, dc) if M > 0 and dc is not None and dc.numel() else None
    out = raster.grad_outputs(L.VARIANT_ALT, fac, P, M, means3D, opacities, scales, rotations, sh, dc, need_cov3D)
    if P != 0:  # P == 0: nothing is launched
        a, keep, P, M = _raster_args(background, means3D, colors, opacities, scales, rotations, scale_modifier,
                                     cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, H, W, dc, sh, degree,
                                     campos, False, antialiasing, debug)
        dinv = None
        if dL_dout_invdepth is not None and dL_dout_invdepth.numel():
            dinv = dL_dout_invdepth.contiguous().float()
        raster.backward(lib, a, keep, out, fac, P, R, radii, geomBuffer, binningBuffer, imageBuffer, dL_dout_color,
                        dinv, degree)
    return (out["dmean2D"], out["dcolor"], out["dopacity"], out["dmean3D"], out["dcov3D"], out["ddc"], out["dsh"],
            out["dscale"], out["drot"])


def adamUpdate(param, param_grad, exp_avg, exp_avg_sq, visible, lr, b1, b2, eps, N, M):
    """In-place sparse Adam step (rasterize_points.cu:255-281, adam.cu:9-36): element p of the N x M parameter
    is updated iff visible[p // M]."""
    lib = L.load()
    for t in (param, param_grad, exp_avg, exp_avg_sq):
        if not t.is_contiguous() or t.dtype != torch.float32:
            raise RuntimeError("adamUpdate expects contiguous float32 tensors (updated in place)")
    vis = visible.contiguous()
    if vis.dtype != torch.bool:
        vis = vis.to(torch.bool)
    L.require_gpu(param, param_grad, exp_avg, exp_avg_sq, vis)
    if int(N) * int(M) > param.numel():
        raise RuntimeError("adamUpdate: N * M exceeds the parameter size")
    L.check(lib.hlgs_adam_update(L.ptr(param), L.ptr(param_grad), L.ptr(exp_avg), L.ptr(exp_avg_sq), L.ptr(vis),
                                 float(lr), float(b1), float(b2), float(eps), int(N), int(M), L.stream()))
