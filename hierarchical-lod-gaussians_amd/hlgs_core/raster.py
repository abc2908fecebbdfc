"""How a frame is driven through libhlgs.so's rasterizer: the binding `diff_gaussian_rasterization._C` and
`alt_gaussian_rasterization._C` share.  Each front end keeps what differs between the two reference extensions (its
argument order, the hierarchy tensors, how P and M are read, its return tuples) and calls in here for the rest.
Tensors are allocated with torch on the inputs' device; every kernel runs inside libhlgs.so (gfx950) on torch's
current stream.
"""
import ctypes as C

import torch

from hlgs_core import _lib as L
from hlgs_core import dp

_vp = C.c_void_p

# Binning buffer sizes, per front end (RasterArgs.variant) and device: see forward().  Each front end's
# `_C._binning_hint` is its dict in here.
binning_hints = {L.VARIANT_HIERARCHY: {}, L.VARIANT_ALT: {}}


def _dev_f32(t, device):
    """Small per-call tensors (bg, view/proj matrices, campos) must live on the device: the kernels
    dereference them (rasterize_points.cu:109-125)."""
    return t.to(device=device, dtype=torch.float32).contiguous()


def _dest(src, shape, f32, late=False):
    """Gradient output for input `src`: the view hlgs_core.dp.direct_grad offers (a view-DP exchange's flat buffer)
    when its shape matches, else a fresh tensor.  Every kernel output row is written, so no zero-fill either way.
    late: the output is completed by the SH backward (dmean3D, dsh, ddc)."""
    d = dp.direct_grad(src, late) if src is not None else None
    return d if d is not None and tuple(d.shape) == tuple(shape) else torch.empty(shape, **f32)


def _opt(t, dtype=None):
    """Empty tensor -> None (NULL, as data_ptr() of an empty tensor is nullptr in the reference); otherwise a
    contiguous view (rasterize_points.cu calls .contiguous())."""
    if t is None or t.numel() == 0:
        return None
    t = t.contiguous()
    if dtype is not None and t.dtype != dtype:
        t = t.to(dtype)
    return t


def raster_args(variant, P, P_full, M, bg, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp,
                viewmatrix, projmatrix, tan_fovx, tan_fovy, H, W, sh, degree, campos, prefiltered, debug,
                antialiasing=1, dc=None, indices=None, parents=None, ts=None, kids=None):
    """-> (L.RasterArgs, keep).  dc and the four hierarchy tensors come normalised (None or contiguous, in the ABI's
    dtype) from the front end that has them; `keep` holds every tensor the struct points into."""
    dev = means3D.device
    keep = dict(bg=_dev_f32(bg, dev), means3D=means3D.contiguous(), colors=_opt(colors), opacity=_opt(opacity),
                scales=_opt(scales), rotations=_opt(rotations), cov3D=_opt(cov3D_precomp),
                view=_dev_f32(viewmatrix, dev), proj=_dev_f32(projmatrix, dev), campos=_dev_f32(campos, dev),
                sh=_opt(sh), dc=dc, indices=indices, parents=parents, ts=ts, kids=kids)
    L.require_gpu(*[v for v in keep.values() if isinstance(v, torch.Tensor)])
    a = L.RasterArgs(P=P, P_full=P_full, D=int(degree), M=M, W=int(W), H=int(H),
                     bg=L.ptr(keep["bg"]), means3D=L.ptr(keep["means3D"]), shs=L.ptr(keep["sh"]),
                     colors_precomp=L.ptr(keep["colors"]), opacities=L.ptr(keep["opacity"]),
                     scales=L.ptr(keep["scales"]), rotations=L.ptr(keep["rotations"]),
                     cov3D_precomp=L.ptr(keep["cov3D"]), viewmatrix=L.ptr(keep["view"]),
                     projmatrix=L.ptr(keep["proj"]), campos=L.ptr(keep["campos"]),
                     scale_modifier=float(scale_modifier), tanfovx=float(tan_fovx), tanfovy=float(tan_fovy),
                     indices=L.ptr(indices), parent_indices=L.ptr(parents), ts=L.ptr(ts), kids=L.ptr(kids),
                     prefiltered=int(bool(prefiltered)), debug=int(bool(debug)), dc=L.ptr(dc),
                     antialiasing=int(bool(antialiasing)), variant=variant)
    return a, keep


def forward(lib, a, hint, P, H, W, dev, do_depth, need_seen):
    """-> (num_rendered, color (3,H,W), invdepth (1 or 0,H,W), radii (P,), geom, binning, img, seen (P,) or None).
    hint: the front end's dict of binning_hints."""
    f32 = dict(dtype=torch.float32, device=dev)
    u8 = dict(dtype=torch.uint8, device=dev)
    color = torch.empty((3, H, W), **f32)
    invdepth = torch.empty((1 if do_depth else 0, H, W), **f32)
    radii = torch.empty((P,), dtype=torch.int32, device=dev)
    seen = torch.empty((P,), dtype=torch.int32, device=dev) if need_seen else None
    geom = torch.empty((lib.hlgs_geom_buffer_size(P),), **u8)
    img = torch.empty((lib.hlgs_image_buffer_size(W, H),), **u8)
    info = L.FrameInfo()
    # The binning buffer is sized from the largest frame seen on this device (+15%), so prepare and render
    # run in one library call; a frame that outgrows it gets an exact buffer and a second call.
    binning = torch.empty((hint.get(dev, 0),), **u8)
    s = L.stream()
    pinv, pseen = L.ptr(invdepth), L.ptr(seen)
    L.check(lib.hlgs_rasterize_forward(C.byref(a), L.ptr(geom), L.ptr(img), L.ptr(radii), L.ptr(binning),
                                       binning.numel(), C.byref(info), L.ptr(color), pinv, pseen, s))
    if not info.rendered:
        need = lib.hlgs_binning_buffer_size(info.num_binned)
        binning = torch.empty((need,), **u8)
        L.check(lib.hlgs_rasterize_forward_render(C.byref(a), L.ptr(radii), L.ptr(geom), L.ptr(img), L.ptr(binning),
                                                  C.byref(info), L.ptr(color), pinv, pseen, s))
        hint[dev] = int(need * 1.15)
    return int(info.num_rendered), color, invdepth, radii, geom, binning, img, seen


def grad_outputs(variant, fac, P, M, means3D, opacities, scales, rotations, sh, dc, need_cov3D):
    """The backward's output tensors by hlgs_grads member.  fac: hlgs_core.dp.colour_factor's tuple, whose views take
    the place of dsh / ddc, or None.  ddc exists in the alt front end only (dc: its degree-0 coefficients)."""
    f32 = dict(dtype=torch.float32, device=means3D.device)
    ddc = None
    if variant == L.VARIANT_ALT:
        ddc = fac[2] if fac is not None else _dest(dc, (P, 1, 3), f32, True)
    return dict(dmean2D=torch.empty((P, 3), **f32), dcolor=torch.empty((P, 3), **f32),
                dopacity=_dest(opacities, (P, 1), f32), dmean3D=_dest(means3D, (P, 3), f32, True),
                dcov3D=torch.empty((P if need_cov3D else 0, 6), **f32), ddc=ddc,
                dsh=fac[1] if fac is not None else _dest(sh, (P, M, 3), f32, True),
                dscale=_dest(scales, (P, 3), f32), drot=_dest(rotations, (P, 4), f32))


def backward(lib, a, keep, out, fac, P, R, radii, geomBuffer, binningBuffer, imageBuffer, dL_dout_color, dinv, degree):
    """Fills `out` (grad_outputs) through hlgs_rasterize_backward_split.  dinv: the inverse-depth gradient as
    contiguous float32, or None."""
    g = L.Grads(**{k: L.ptr(v) for k, v in out.items()}, drgb=L.ptr(fac[0]) if fac is not None else None)
    dpix = dL_dout_color.contiguous().float()
    scratch = torch.empty((lib.hlgs_backward_scratch_size(P, int(R)),), dtype=torch.uint8,
                          device=keep["means3D"].device)
    # the SH backward on an overlapping exchange's late stream (hlgs_core.dp.late_stream_for), else in order
    late = dp.late_stream_for(out["dmean3D"], out["ddc"], out["dsh"])
    L.check(lib.hlgs_rasterize_backward_split(C.byref(a), L.ptr(radii.contiguous()), L.ptr(geomBuffer),
                                              L.ptr(imageBuffer), L.ptr(binningBuffer), int(R), L.ptr(scratch),
                                              L.ptr(dpix), L.ptr(dinv), C.byref(g), L.stream(),
                                              _vp(late.cuda_stream) if late is not None else None))
    if late is not None:
        dp.note_late_work(late, list(keep.values()) + list(out.values()) +
                          [radii, geomBuffer, imageBuffer, binningBuffer, scratch, dpix, dinv])
    if fac is not None:
        fac[3](keep["campos"], degree, a.variant)


def mark_visible(means3D, viewmatrix, projmatrix):
    """z > 0.2 view-space test per point (hierarchy-rasterizer rasterizer_impl.cu:54-66; alt-rasterizer
    rasterizer_impl.cu:104-116, 235-247, rasterize_points.cu:234-253) -> bool tensor."""
    lib = L.load()
    dev = means3D.device
    m = means3D.contiguous().float()
    L.require_gpu(m)
    present = torch.zeros((m.size(0),), dtype=torch.bool, device=dev)
    view, proj = _dev_f32(viewmatrix, dev), _dev_f32(projmatrix, dev)
    L.check(lib.hlgs_mark_visible(m.size(0), L.ptr(m), L.ptr(view), L.ptr(proj), L.ptr(present), L.stream()))
    return present


def compute_relocation(opacity_old, scale_old, N, binoms, n_max):
    """MCMC relocation (hierarchy-rasterizer rasterize_points.cu:248-271; alt-rasterizer rasterize_points.cu:284-306)
    -> (opacity (P,), scale (3P,))."""
    lib = L.load()
    o = opacity_old.contiguous().float()
    s = scale_old.contiguous().float()
    n = N.contiguous().to(torch.int32)
    b = binoms.contiguous().float()
    L.require_gpu(o, s, n, b)
    P = o.size(0)
    new_o = torch.zeros((P,), dtype=torch.float32, device=o.device)
    new_s = torch.zeros((3 * P,), dtype=torch.float32, device=o.device)
    L.check(lib.hlgs_compute_relocation(P, L.ptr(o), L.ptr(s), L.ptr(n), L.ptr(b), int(n_max), L.ptr(new_o),
                                        L.ptr(new_s), L.stream()))
    return new_o, new_s
