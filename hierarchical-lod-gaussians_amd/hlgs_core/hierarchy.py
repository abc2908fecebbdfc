"""The dynamic hierarchy of a set of flat Gaussians, built on the GPU: the step the reference runs offline as
GaussianHierarchyCreator (submodules/gaussianhierarchy/mainHierarchyCreator.cpp) between a trained chunk and
train_post.py.

  valid_gaussian_mask(...)      the creator's filter (mainHierarchyCreator.cpp:87-152) as a bool tensor
  build_dynamic_hierarchy(...)  kd-tree, bottom-up merge, top-down rotation alignment and the pre-order node table
                                (hlgs_hier_build, include/hlgs.h), returned as load_dynamic_hierarchy returns a file

Inputs are activated Gaussians (opacity in (0, 1], scales = exp(stored), rotations in any norm) without the skybox
rows: slice those off first, as the creator's `skyboxpoints` argument does.  What differs from the reference is
listed in DESIGN.md §6 (A-33 to A-37).
"""
import torch

from hlgs_core import _lib as L

LDS_CAP = 2048          # HLGS_HIER_LDS_CAP: leaves of a subtree one workgroup finishes on its own
MAX_N = 1 << 30         # HLGS_HIER_MAX_N
STAGES = ("kd_top", "kd_lds", "leaves", "merge", "align", "finish")
_INVALID, _NAN, _BUMP = 1, 2, 4


def _inputs(xyz, shs, opacity, scales, rotations):
    """The five inputs as contiguous float32 tensors of N rows; shs flattened to (N, sh_floats)."""
    N = int(xyz.shape[0])
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError("xyz must have dimensions (N, 3)")
    if N == 0:
        raise ValueError("a hierarchy needs at least one Gaussian (N = 0)")
    if N > MAX_N:
        raise ValueError(f"N = {N} exceeds {MAX_N}: the 2N - 1 node ids are int32")
    c = lambda t: t.detach().to(torch.float32).contiguous()  # noqa: E731
    xyz, shs, opacity, scales, rotations = c(xyz), c(shs), c(opacity), c(scales), c(rotations)
    for t, w, name in ((opacity, 1, "opacity"), (scales, 3, "scales"), (rotations, 4, "rotations")):
        if t.numel() != N * w:
            raise ValueError(f"{name} must hold {N} x {w} values")
    if shs.shape[0] != N or shs.numel() == 0:
        raise ValueError("shs must hold N non-empty rows")
    return N, xyz, shs, opacity, scales, rotations


def valid_gaussian_mask(xyz, shs, opacity, scales, rotations):
    """(N,) bool, on the device: the rows the creator keeps (mainHierarchyCreator.cpp:87-152) -- opacity neither inf,
    NaN nor exactly 0, no scale above 10, no NaN in scale, rotation, position or SH."""
    N, xyz, shs, opacity, scales, rotations = _inputs(xyz, shs, opacity, scales, rotations)
    L.require_gpu(xyz, shs, opacity, scales, rotations)
    mask = torch.empty((N,), dtype=torch.uint8, device=xyz.device)
    L.check(L.load().hlgs_hier_valid_mask(N, shs.numel() // N, L.ptr(xyz), L.ptr(shs), L.ptr(opacity), L.ptr(scales),
                                          L.ptr(rotations), L.ptr(mask), L.stream()))
    return mask.bool()


def build_dynamic_hierarchy(xyz, shs, opacity, scales, rotations, *, stage_ms=None):
    """The creator's hierarchy over N activated Gaussians (device tensors: xyz (N, 3), shs (N, K, 3) or (N, 3 K),
    opacity (N,) or (N, 1), scales (N, 3), rotations (N, 4) as (w, x, y, z), normalised here).  Returns (pos (G, 3),
    shs (G, K, 3), alpha (G, 1), log_scales (G, 3), rot (G, 4), nodes (G, 6) int32) on the device with G = 2N - 1,
    in pre-order with row id == node id: what load_dynamic_hierarchy returns for the creator's file, ready for
    write_dynamic_hierarchy and hlgs_core.scene.assemble_hierarchy.  nodes[:, 5] of a leaf is its input row.
    Raises ValueError for N = 0 and for rows holding a non-finite value or opacity 0 (filter with
    valid_gaussian_mask first), RuntimeError where the reference's eigen-solve throws (a NaN eigenvalue).
    stage_ms: a dict that receives the event time of every stage (the stages are then run one call each)."""
    N, xyz, shs, opacity, scales, rotations = _inputs(xyz, shs, opacity, scales, rotations)
    L.require_gpu(xyz, shs, opacity, scales, rotations)
    lib = L.load()
    dev = xyz.device
    shf = shs.numel() // N
    G = 2 * N - 1
    f = lambda *sh: torch.empty(sh, dtype=torch.float32, device=dev)  # noqa: E731
    pos, out_shs, alpha, log_scales, rot = f(G, 3), f(G, shf), f(G, 1), f(G, 3), f(G, 4)
    nodes = torch.empty((G, 6), dtype=torch.int32, device=dev)
    scratch = torch.empty((lib.hlgs_hier_scratch_size(N) + 256,), dtype=torch.uint8, device=dev)
    scratch = scratch[-scratch.data_ptr() % 256:]

    def run(stages):
        L.check(lib.hlgs_hier_build(N, shf, L.ptr(xyz), L.ptr(shs), L.ptr(opacity), L.ptr(scales), L.ptr(rotations),
                                    L.ptr(pos), L.ptr(out_shs), L.ptr(alpha), L.ptr(log_scales), L.ptr(rot),
                                    L.ptr(nodes), L.ptr(scratch), stages, L.stream()))

    if stage_ms is None:
        run(0x3f)
    else:
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(STAGES) + 1)]
        ev[0].record()
        for i in range(len(STAGES)):
            run(1 << i)
            ev[i + 1].record()
    status = int(scratch[:4].view(torch.int32).cpu()[0])  # the build's one read-back
    if stage_ms is not None:
        stage_ms.update({n: ev[i].elapsed_time(ev[i + 1]) for i, n in enumerate(STAGES)})
    if status & _INVALID:
        raise ValueError("build_dynamic_hierarchy: a row holds a non-finite value or has opacity 0 "
                         "(valid_gaussian_mask gives the rows the creator keeps)")
    if status & _NAN:
        raise RuntimeError("build_dynamic_hierarchy: Found Nans! (an eigenvalue of a merged covariance is NaN)")
    if status & _BUMP:
        raise RuntimeError("build_dynamic_hierarchy: a merged covariance kept a zero eigenvalue after 16 diagonal "
                           "bumps")
    shape = tuple(shs.shape[1:]) if shs.dim() == 3 and shs.shape[2] == 3 else (shf // 3, 3) if shf % 3 == 0 else (shf,)
    return pos, out_shs.reshape(G, *shape), alpha, log_scales, rot, nodes
