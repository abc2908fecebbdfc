"""`simple_knn._C`: distCUDA2 through libhlgs.so (csrc/knn.hip, include/hlgs.h hlgs_knn_mean_dist2).

distCUDA2(points) is the mean of the squared distances from every point to its three nearest other points, in float32
and equal bit for bit to the all-pairs evaluation of (dx*dx + dy*dy) + dz*dz; with fewer than three other points the
result is +inf.  There is no CPU path.
"""
import torch

from hlgs_core import _lib as L

# include/hlgs.h HLGS_KNN_BOX, HLGS_KNN_SUPER, HLGS_KNN_SORT_TILE (tests/test_knn_cpu.py compares them with the header)
BOX = 64            # Morton-sorted points per box: one wave of the search
SUPER = 64          # boxes per super-box
SORT_TILE = 1024    # keys one block of a radix pass handles
RADIX = 256         # digits per pass (csrc/knn.hip kRadixBits = 8): the scan runs over RADIX * sort_tiles counts
SCAN_ITEMS = 2048   # counts one block of the scan handles (csrc/hlgs_internal.h kScanItems)
BBOX_BLOCKS = 256   # most blocks of the bounding-box reduction, 256 points each per stride (csrc/knn.hip kBoxParts)


def plan(P):
    """The sizes that pick the code paths of one call: boxes and super-boxes of the search and the steps of 64
    super-boxes each wave tests (above one, the step's base index is non-zero), tiles of the radix sort, the levels of
    the scan over its digit counts (1: a single block), and the strides each block of the bounding-box reduction takes
    (the bounding box only shapes the Morton keys, so it can change the time of a call and never its result)."""
    P = int(P)
    boxes = -(-P // BOX)
    tiles = -(-P // SORT_TILE)
    n, levels = RADIX * tiles, 1 if P else 0
    while n > SCAN_ITEMS:
        n = -(-n // SCAN_ITEMS)
        levels += 1
    supers = -(-boxes // SUPER)
    return dict(boxes=boxes, super_boxes=supers, super_steps=-(-supers // 64), sort_tiles=tiles, scan_levels=levels,
                bbox_strides=-(-P // (256 * BBOX_BLOCKS)))


def distCUDA2(points):
    """(P, 3) device tensor -> (P,) float32: mean squared distance to the three nearest other points."""
    p = points.detach().contiguous().float()
    if p.dim() != 2 or p.size(1) != 3:
        raise RuntimeError("points must have dimensions (num_points, 3)")
    L.require_gpu(p)
    if not p.is_cuda:
        raise RuntimeError("libhlgs expects device tensors")
    P = p.size(0)
    out = torch.empty((P,), dtype=torch.float32, device=p.device)
    if P == 0:
        return out
    lib = L.load()
    with torch.cuda.device(p.device):
        scratch = torch.empty((int(lib.hlgs_knn_scratch_size(P)),), dtype=torch.uint8, device=p.device)
        L.check(lib.hlgs_knn_mean_dist2(P, L.ptr(p), L.ptr(scratch), L.ptr(out), L.stream()))
    return out
