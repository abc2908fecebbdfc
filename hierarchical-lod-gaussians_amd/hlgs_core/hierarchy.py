"""The dynamic hierarchy of a set of flat Gaussians, built on the GPU: the step the reference runs offline as
GaussianHierarchyCreator (submodules/gaussianhierarchy/mainHierarchyCreator.cpp) between a trained chunk and
train_post.py.

  valid_gaussian_mask(...)      the creator's filter (mainHierarchyCreator.cpp:87-152) as a bool tensor
  build_dynamic_hierarchy(...)  kd-tree, bottom-up merge, top-down rotation alignment and the pre-order node table
                                (hlgs_hier_build, include/hlgs.h), returned as load_dynamic_hierarchy returns a file

  merge_dynamic_hierarchies(...)  K trained chunk hierarchies and their chunk centres become one scene hierarchy
                                (hlgs_hier_merge_*, include/hlgs.h): the offline GaussianHierarchyMerger
  merge_hierarchy_files(...)    the same from .dhier files to a .dhier file

Inputs are activated Gaussians (opacity in (0, 1], scales = exp(stored), rotations in any norm) without the skybox
rows: slice those off first, as the creator's `skyboxpoints` argument does.  What differs from the reference is
listed in DESIGN.md §6 (A-33 to A-41).
"""
import ctypes as C

import numpy as np
import torch

from hlgs_core import _lib as L

LDS_CAP = 2048          # HLGS_HIER_LDS_CAP: leaves of a subtree one workgroup finishes on its own
MAX_N = 1 << 30         # HLGS_HIER_MAX_N
STAGES = ("kd_top", "kd_lds", "leaves", "merge", "align", "finish")
_INVALID, _NAN, _BUMP = 1, 2, 4
MERGE_MAX_DEPTH = 2047  # HLGS_MERGE_MAX_DEPTH
MERGE_STAGES = ("validate", "weights", "bottom_up", "top_down", "scatter")
_MERGE_HEADER = 8       # HLGS_MERGE_HEADER_INTS
_LINKS, _ROOT = 1, 2


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


def _chunk_shape(k, chunk):
    """(n, SH floats per row, SH shape) of chunk k after checking that its six arrays belong together."""
    if len(chunk) != 6:
        raise ValueError(f"chunk {k}: expected (pos, shs, alpha, log_scales, rot, nodes), as load_dynamic_hierarchy "
                         "returns them")
    pos, shs, alpha, log_scales, rot, nodes = chunk
    n = int(pos.shape[0])
    if pos.dim() != 2 or pos.shape[1] != 3:
        raise ValueError(f"chunk {k}: pos must have dimensions (n, 3)")
    if n < 1 or n > MAX_N:
        raise ValueError(f"chunk {k}: n = {n} is outside [1, {MAX_N}]")
    for t, w, name in ((alpha, 1, "alpha"), (log_scales, 3, "log_scales"), (rot, 4, "rot"), (nodes, 6, "nodes")):
        if t.numel() != n * w:
            raise ValueError(f"chunk {k}: {name} must hold {n} x {w} values")
    if shs.shape[0] != n or shs.numel() == 0:
        raise ValueError(f"chunk {k}: shs must hold n non-empty rows")
    return n, shs.numel() // n, tuple(shs.shape[1:])


def _chunk_on(dev, chunk):
    """The six arrays as contiguous device tensors: float32, and int32 for the node table."""
    return tuple(t.detach().to(device=dev, dtype=torch.int32 if i == 5 else torch.float32).contiguous()
                 for i, t in enumerate(chunk))


def merge_dynamic_hierarchies(chunks, centers, *, falloff=0.05, root_scale=1e4, stage_ms=None):
    """K trained chunk hierarchies become one scene hierarchy: the reference's GaussianHierarchyMerger
    (hierarchy_explicit_loader.cpp:22-150, mainHierarchyMerger.cpp:94-140, writer.cpp:99-171) on the GPU, as
    include/hlgs.h (hlgs_hier_merge_*) restates it.

    chunks: K 6-tuples (pos (n, 3), shs (n, C, 3), alpha (n, 1) activated, log_scales (n, 3), rot (n, 4), nodes (n, 6)
    int32) as load_dynamic_hierarchy returns them, device or CPU tensors, without skybox rows.  Row 0 is the chunk's
    root; the other rows may be in any order (train_post's MCMC round appends and rewires rows) and a node may have any
    number of children.  centers: (K, 3), the chunks' center.txt.

    Every node is weighted by its distance to its own and to the nearest other centre (1 inside the chunk, 0 beyond
    (1 + falloff) x the distance to the other centre, linear between); weight-0 nodes are dropped, their children
    spliced into the child list of the nearest kept ancestor; a kept node's opacity is scaled by its weight and the
    rest of its row copied bit for bit; the chunk root moves to the centre; the chunks are re-linearised in pre-order
    under one new root (row 0: DESIGN.md §6 A-40), whose scale `root_scale` no cut selects.  K = 1 keeps everything.

    Returns (pos, shs, alpha, log_scales, rot, nodes, chunk_roots) on the device: the 6-tuple, ready for
    write_dynamic_hierarchy, hlgs_core.scene.assemble_hierarchy and the LOD cut (expand_to_size_dynamic,
    get_interpolation_weights_dynamic, interpolate_lod, which go by parent pointers and the parent's child_count and
    so take any child count), and the K chunk roots' ids (int32).  nodes[:, 5] of a kept input-leaf is its rank among
    the kept input-leaves, -1 elsewhere.  The reference's SPT walk (cut_hierarchy_on_condition,
    scene/gaussian_model.py:386-389) visits exactly two children per node and cannot take this result; the SPT path's
    n-ary mode (hlgs_core.spt.build_hierarchical_spt_device(..., nary=True), then SPTCache) streams it as it is.

    Raises ValueError for chunks of different SH width, non-finite centres (a chunk whose root is dropped), a malformed
    node table (an index out of range, a child list shorter than child_count, a child naming another parent, a row in
    two lists or none, a depth that is not its parent's + 1, a depth above 2047).  One read-back per chunk (kept nodes,
    kept leaves, status, rows per depth); everything else is queued on the current stream.
    stage_ms: a dict that receives the event time of every stage, summed over the chunks (the stages are then run one
    call each)."""
    chunks = list(chunks)
    K = len(chunks)
    if K < 1:
        raise ValueError("merge_dynamic_hierarchies needs at least one chunk")
    dev = next((t.device for ch in chunks for t in ch if t.is_cuda), torch.device("cuda"))
    cen = torch.as_tensor(np.asarray(centers.detach().cpu() if torch.is_tensor(centers) else centers, np.float32))
    if tuple(cen.shape) != (K, 3):
        raise ValueError(f"centers must have dimensions ({K}, 3)")
    if not bool(torch.isfinite(cen).all()):
        raise ValueError("merge_dynamic_hierarchies: a chunk centre is not finite (its chunk's root would be dropped)")
    shapes = [_chunk_shape(k, ch) for k, ch in enumerate(chunks)]
    shf, sh_shape = shapes[0][1], shapes[0][2]
    if any(sh[1] != shf for sh in shapes):
        raise ValueError("all chunks must share one SH width")
    L.require_gpu()
    cs = [sh + _chunk_on(dev, ch) for sh, ch in zip(shapes, chunks)]
    lib = L.load()
    cen = cen.to(dev).contiguous()
    timed = stage_ms is not None
    marks = []

    def staged(fn, names, bits):
        """fn(stages) for all stages at once, or one call per stage between events."""
        if not timed:
            fn(sum(bits))
            return
        for name, bit in zip(names, bits):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(bit)
            e1.record()
            marks.append((name, e0, e1))

    scratch = []
    for k, (n, _, _, pos, shs, alpha, log_scales, rot, nodes) in enumerate(cs):
        sc = torch.empty((lib.hlgs_hier_merge_scratch_size(n) + 256,), dtype=torch.uint8, device=dev)
        sc = sc[-sc.data_ptr() % 256:]
        scratch.append(sc)
        staged(lambda st: L.check(lib.hlgs_hier_merge_plan(n, k, K, L.ptr(cen), L.ptr(pos), L.ptr(nodes), float(falloff),
                                                           L.ptr(sc), st, L.stream())), MERGE_STAGES[:2], (1, 2))
    words = _MERGE_HEADER + MERGE_MAX_DEPTH + 1
    heads = [sc[:4 * words].view(torch.int32).cpu().numpy() for sc in scratch]  # the one read-back per chunk
    for k, h in enumerate(heads):
        if h[0] & _LINKS:
            raise ValueError(f"merge_dynamic_hierarchies: chunk {k}'s node table is malformed (an index out of range, "
                             "a child list that does not match child_count, parent or depth, or a depth above "
                             f"{MERGE_MAX_DEPTH})")
        if h[0] & _ROOT:
            raise ValueError(f"merge_dynamic_hierarchies: chunk {k}'s root is dropped (a non-finite centre)")
    kept = [int(h[1]) for h in heads]
    leaves = [int(h[2]) for h in heads]
    G = 1 + sum(kept)
    if G >= 1 << 31:
        raise ValueError(f"the merged hierarchy would hold {G} rows; node ids are int32")
    f = lambda *sh: torch.empty(sh, dtype=torch.float32, device=dev)  # noqa: E731
    pos_o, shs_o, alpha_o, ls_o, rot_o = f(G, 3), f(G, shf), f(G, 1), f(G, 3), f(G, 4)
    nodes_o = torch.empty((G, 6), dtype=torch.int32, device=dev)
    outs = [L.ptr(t) for t in (pos_o, shs_o, alpha_o, ls_o, rot_o, nodes_o)]
    offs = np.concatenate([[1], 1 + np.cumsum(kept)]).astype(np.int64)
    loffs = np.concatenate([[0], np.cumsum(leaves)]).astype(np.int64)
    for k, (n, _, _, pos, shs, alpha, log_scales, rot, nodes) in enumerate(cs):
        levels = np.ascontiguousarray(heads[k][_MERGE_HEADER:], np.int32)
        lv = levels.ctypes.data_as(C.c_void_p)
        staged(lambda st: L.check(lib.hlgs_hier_merge_emit(n, shf, k, K, L.ptr(cen), L.ptr(pos), L.ptr(shs),
                                                           L.ptr(alpha), L.ptr(log_scales), L.ptr(rot), L.ptr(nodes),
                                                           lv, kept[k], int(offs[k]), int(loffs[k]), G, *outs,
                                                           L.ptr(scratch[k]), st, L.stream())),
               MERGE_STAGES[2:], (1, 2, 4))
    chunk_roots = torch.tensor(offs[:K], dtype=torch.int32).to(dev)
    L.check(lib.hlgs_hier_merge_root(K, shf, G, L.ptr(chunk_roots), L.ptr(cen), float(root_scale), *outs, L.stream()))
    if timed:
        torch.cuda.current_stream().synchronize()
        for name in MERGE_STAGES:
            stage_ms[name] = sum(e0.elapsed_time(e1) for nm, e0, e1 in marks if nm == name)
    shape = sh_shape if len(sh_shape) == 2 and sh_shape[1] == 3 else (shf // 3, 3) if shf % 3 == 0 else (shf,)
    return pos_o, shs_o.reshape(G, *shape), alpha_o, ls_o, rot_o, nodes_o, chunk_roots


def merge_hierarchy_files(hier_paths, centers, out_path, SH_degree):
    """The file-level step: load_dynamic_hierarchy every path of hier_paths, merge_dynamic_hierarchies with `centers`
    ((K, 3) values, or K paths of center.txt files holding three numbers each) and write_dynamic_hierarchy the result
    to out_path with SH_degree.  Returns what merge_dynamic_hierarchies returns."""
    from gaussian_hierarchy import load_dynamic_hierarchy, write_dynamic_hierarchy
    import os
    if not torch.is_tensor(centers) and not isinstance(centers, np.ndarray):
        centers = [np.loadtxt(c, dtype=np.float32).reshape(-1)[:3] if isinstance(c, (str, bytes, os.PathLike)) else c
                   for c in centers]
    chunks = [load_dynamic_hierarchy(p) for p in hier_paths]
    out = merge_dynamic_hierarchies(chunks, np.asarray(centers, np.float32))
    write_dynamic_hierarchy(out_path, *out[:6], SH_degree)
    return out
