"""`diff_gaussian_rasterization._C` on MI355X.

Same entry points, argument order and return tuples as the reference extension
(submodules/hierarchy-rasterizer/ext.cpp:15-19, rasterize_points.cu:36-271), plus `mark_visible`, which
the reference's Python wrapper calls (__init__.py:174) but never binds.  Tensors are
allocated with torch on the current device; every kernel runs inside libhlgs.so (gfx950) on torch's
current stream.
"""
import torch

from hlgs_core import _lib as L
from hlgs_core import dp
from hlgs_core import raster
from hlgs_core.raster import compute_relocation, mark_visible  # noqa: F401  (rasterize_points.cu:248-271; A-2)


def _raster_args(bg, render_indices, parent_indices, ts, kids, means3D, colors, opacity, scales, rotations,
                 scale_modifier, cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, H, W, sh, degree,
                 campos, prefiltered, debug):
    if means3D.ndimension() != 2 or means3D.size(1) != 3:
        raise RuntimeError("means3D must have dimensions (num_points, 3)")
    indices = raster._opt(render_indices, torch.int32)
    P_full = means3D.size(0)
    P = indices.size(0) if indices is not None else P_full
    M = sh.size(1) if (sh is not None and sh.numel() and sh.size(0) != 0) else 0
    a, keep = raster.raster_args(L.VARIANT_HIERARCHY, P, P_full, M, bg, means3D, colors, opacity, scales, rotations,
                                 scale_modifier, cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, H, W, sh,
                                 degree, campos, prefiltered, debug, indices=indices,
                                 parents=raster._opt(parent_indices, torch.int32), ts=raster._opt(ts, torch.float32),
                                 kids=raster._opt(kids, torch.int32))
    return a, keep, P, P_full, M


_binning_hint = raster.binning_hints[L.VARIANT_HIERARCHY]


def rasterize_gaussians(bg, render_indices, parent_indices, ts, kids, means3D, colors, opacity, scales, rotations,
                        scale_modifier, cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, image_height,
                        image_width, sh, degree, campos, prefiltered, debug, do_depth, *, need_seen=True):
    """-> (num_rendered, color, radii, geomBuffer, binningBuffer, imgBuffer, invdepth, seen)
    (rasterize_points.cu:36-139).  need_seen=False (used by the autograd wrapper, which drops it) returns an empty
    `seen` and skips its per-splat stores."""
    lib = L.load()
    H, W = int(image_height), int(image_width)
    a, keep, P, _, _ = _raster_args(bg, render_indices, parent_indices, ts, kids, means3D, colors, opacity, scales,
                                    rotations, scale_modifier, cov3D_precomp, viewmatrix, projmatrix, tan_fovx,
                                    tan_fovy, H, W, sh, degree, campos, prefiltered, debug)
    dev = means3D.device
    n, color, invdepth, radii, geom, binning, img, seen = raster.forward(lib, a, _binning_hint, P, H, W, dev,
                                                                         do_depth, need_seen)
    if seen is None:
        seen = torch.empty((0,), dtype=torch.int32, device=dev)
    return n, color, radii, geom, binning, img, invdepth, seen


def rasterize_gaussians_backward(bg, render_indices, parent_indices, ts, kids, means3D, radii, colors, opacities,
                                 scales, rotations, scale_modifier, cov3D_precomp, viewmatrix, projmatrix, tan_fovx,
                                 tan_fovy, dL_dout_color, dL_dout_invdepth, sh, degree, campos, geomBuffer, R,
                                 binningBuffer, imageBuffer, debug, *, need_cov3D=True):
    """-> (dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations)
    (rasterize_points.cu:141-245).  need_cov3D=False (the autograd wrapper without cov3D_precomp) returns an empty
    dL_dcov3D and skips writing its rows."""
    lib = L.load()
    H, W = int(dL_dout_color.size(1)), int(dL_dout_color.size(2))
    a, keep, P, P_full, M = _raster_args(bg, render_indices, parent_indices, ts, kids, means3D, colors, opacities,
                                         scales, rotations, scale_modifier, cov3D_precomp, viewmatrix, projmatrix,
                                         tan_fovx, tan_fovy, H, W, sh, degree, campos, False, debug)
    # a colour-factored view-DP exchange takes dL/dRGB instead of the SH gradient (hlgs_core.dp.colour_factor)
    fac = dp.colour_factor(sh) if M > 0 and keep["indices"] is None else None
    out = raster.grad_outputs(L.VARIANT_HIERARCHY, fac, P_full, M, means3D, opacities, scales, rotations, sh, None,
                              need_cov3D)
    dinv = None
    if dL_dout_invdepth is not None and dL_dout_invdepth.numel() and dL_dout_invdepth.size(0) != 0:
        dinv = dL_dout_invdepth.contiguous().float()
    raster.backward(lib, a, keep, out, fac, P, R, radii, geomBuffer, binningBuffer, imageBuffer, dL_dout_color, dinv,
                    degree)
    return (out["dmean2D"], out["dcolor"], out["dopacity"], out["dmean3D"], out["dcov3D"], out["dsh"], out["dscale"],
            out["drot"])


def _field(buf, offset, count, dtype):
    base = buf.data_ptr()
    shift = ((base + 255) & ~255) - base
    nbytes = count * torch.tensor([], dtype=dtype).element_size()
    return buf[shift + offset: shift + offset + nbytes].view(dtype)


def inspect_point_list(binningBuffer, R, P=0):
    """Sorted per-tile Gaussian ids (tile-major, front to back) held in a forward's binning buffer of a P-Gaussian
    forward (the stored entries carry a footprint quadrant mask below the id: hlgs_point_list_entry_shift)."""
    lib = L.load()
    raw = _field(binningBuffer, lib.hlgs_binning_point_list_offset(int(R)), int(R), torch.int32)
    return (raw.to(torch.int64) & 0xFFFFFFFF) >> lib.hlgs_point_list_entry_shift(int(P))


def inspect_ranges(imageBuffer, W, H):
    """[start, end) of every tile's list (tiles row-major) held in a forward's image buffer."""
    T = ((W + 15) // 16) * ((H + 15) // 16)
    return _field(imageBuffer, L.load().hlgs_image_ranges_offset(int(W), int(H)), 2 * T, torch.int32).view(T, 2)


def inspect_splats(geomBuffer, P):
    """(P, 16) float32 per-Gaussian blend records held in a forward's geometry buffer:
    [0:4] x, y, conic a, b | [4:8] conic c, opacity, r, g | [8:12] b, 1/depth, t, 1/kids |
    [12:16] 0 (unused), x0 | y0 << 16 (int bits), rect width (int bits), alpha threshold on e2
    (csrc/hlgs_internal.h, Geom::splat; a culled Gaussian's record is unspecified)."""
    return _field(geomBuffer, L.load().hlgs_geom_splat_offset(int(P)), 16 * int(P), torch.float32).view(int(P), 16)
