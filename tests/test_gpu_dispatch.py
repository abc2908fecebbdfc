"""The rasterizer's kernel-selection thresholds, each from both sides, against the oracle (DESIGN.md section 3 lists
which test sits on which threshold).

The forward and the backward pick their kernels from sizes only a few frames hit:
- the longest per-tile list picks the tile sort (one-wave register sort <= 1,024 entries, LDS block sort <= 4,096, then
  merge passes whose count and keys / keys2 parity flip at 8,192 and 16,384), the backward's chunking (bwd_chunk_len:
  one chunk up to 192 entries, two up to 384, three of 192 up to 576, three longer ones above) and the blends' 64-splat
  batch count.  helpers.one_tile_scene puts exactly n entries on one tile; the frame's own max_tile_count proves it.
- the Gaussian count P picks the binning block (bin_gauss: 1,024 Gaussians up to P = 786,432, 4,096 above) and, through
  nb = ceil(P / bin_gauss), the code path of k_tile_offsets_plan / k_tile_offsets (registers <8> for nb <= 256, <24> for
  nb <= 768, a loop above).  helpers.sparse_scene makes P as large as the threshold needs while only a few thousand
  Gaussians reach the frame; hlgs_set_plan_polls(0) forces the two-launch re-plan, proven by the image buffer's
  misc[5].
- the previous frame's longest list (Readback::last_maxc, capi.hip) picks the sorts the speculative render queues: one
  test walks all nine ordered transitions in one process and one thread.
- every binding launches on torch's current stream: one test runs them on a side stream behind a long kernel.

Every oracle frame is run with drop_empty=drops_empty(P); tests/test_dispatch_scenes_cpu.py asserts the scenes'
properties from the oracle alone, and the tests here repeat the cheap ones on their own oracle frame.  Tolerances are
the suite's: image 1e-4 with no pixel over (image_check), gradients 1e-3 and element-wise (assert_grad), lists
bit-exact.
"""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

from hlgs_core import _lib as L
from hlgs_core import synthetic as S
from oracle import oracle as O
from helpers import (assert_grad, bin_gauss, binned, drops_empty, equal_depths, image_check, one_tile_scene,
                     sparse_scene, tile_counts)
from test_dispatch_scenes_cpu import (CHUNK_N, CHUNK_N_ALT, ORDER_N, SORT_N, SORT_N_SMALL, SPARSE, SPARSE_WH, TIE_N)

pytestmark = pytest.mark.gpu
DEV = "cuda"
GRADS = ("dmean3D", "dmean2D", "dopacity", "dscale", "drot", "dsh", "ddc")
LISTS = ("ranges", "point_list", "n_contrib")
K_MISC_FAIL = 5  # Img::misc word a timed-out look-back of the fused plan sets (csrc/hlgs_internal.h kMiscFail)


def _upload(a):
    return torch.tensor(np.ascontiguousarray(a), device=DEV) if isinstance(a, np.ndarray) else a.to(DEV)


def _front_end(alt):
    if alt:
        import alt_gaussian_rasterization as M
    else:
        import diff_gaussian_rasterization as M
    return M


def _gpu(sc, cam, grads=None, do_depth=True, up=_upload):
    """One frame through the public API of the scene's front end (GaussianRasterizer of diff_gaussian_rasterization,
    or of alt_gaussian_rasterization for an alt scene), with the backward when `grads` is given.  The frame's tile
    lists, n_contrib and misc words are read from the buffers its autograd node saved.  up: host array or tensor ->
    device tensor (the stream test makes them on its own stream)."""
    from diff_gaussian_rasterization import _C as HC
    alt = bool(sc.get("alt"))
    M = _front_end(alt)
    lib = L.load()
    W, H, P, deg = cam["W"], cam["H"], sc["means3D"].shape[0], sc["sh_degree"]
    leaf = lambda a: up(a).detach().requires_grad_(True)  # noqa: E731
    means3D, opac, scales, rots, shs = (leaf(sc[k]) for k in ("means3D", "opacities", "scales", "rotations", "shs"))
    means2D = torch.zeros_like(means3D, requires_grad=True)
    common = dict(image_height=H, image_width=W, tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"], bg=up(cam["bg"]),
                  scale_modifier=1.0, viewmatrix=up(cam["viewmatrix"]), projmatrix=up(cam["projmatrix"]), sh_degree=deg,
                  campos=up(cam["campos"]), prefiltered=False, debug=False)
    ins = dict(dmean3D=means3D, dmean2D=means2D, dopacity=opac, dscale=scales, drot=rots, dsh=shs)
    if alt:
        ins["ddc"] = dc = leaf(sc["dc"])
        rast = M.GaussianRasterizer(M.GaussianRasterizationSettings(antialiasing=sc["antialiasing"], **common))
        color, radii, invd = rast(means3D=means3D, means2D=means2D, opacities=opac, scales=scales, rotations=rots,
                                  dc=dc, shs=shs)
        geom, binning, img = color.grad_fn.saved_tensors[-4:-1]
    else:
        e_i = torch.empty(0, dtype=torch.int32, device=DEV)
        e_f = torch.empty(0, dtype=torch.float32, device=DEV)
        rast = M.GaussianRasterizer(M.GaussianRasterizationSettings(
            render_indices=e_i, parent_indices=e_i, interpolation_weights=e_f, num_node_kids=e_i, do_depth=do_depth,
            **common))
        color, radii, invd = rast(means3D=means3D, means2D=means2D, opacities=opac, shs=shs, scales=scales,
                                  rotations=rots)
        geom, binning, img = color.grad_fn.saved_tensors[-3:]
    N = W * H
    # the words the plan defines (include/hlgs.h hlgs_image_misc_offset); the rest of the 16 is never written
    misc = HC._field(img, lib.hlgs_image_misc_offset(W, H), 16, torch.int32).cpu().numpy().astype(np.int64)[:6]
    out = dict(num_rendered=int(color.grad_fn.num_rendered), misc=misc,
               ranges=HC.inspect_ranges(img, W, H).cpu().numpy().astype(np.uint32),
               point_list=HC.inspect_point_list(binning, int(misc[0]), P).cpu().numpy().astype(np.uint32),
               n_contrib=HC._field(img, (4 * N + 255) // 256 * 256, N, torch.int32).cpu().numpy())
    if grads is not None:
        g, gd = grads
        loss = (color * up(g)).sum()
        if invd.numel() and gd is not None:
            loss = loss + (invd * up(gd)).sum()
        loss.backward()
        for k, v in ins.items():
            out[k] = v.grad.cpu().numpy()
    out.update(color=color.detach().cpu().numpy(), radii=radii.cpu().numpy(), invdepth=invd.detach().cpu().numpy())
    return out


def _ref(sc, cam, grads=None, do_depth=True):
    """The oracle's frame of the same scene, run with the drop_empty a GPU frame started now has (drops_empty)."""
    alt = bool(sc.get("alt"))
    P = sc["means3D"].shape[0]
    s = dict(sc)
    fr = O.forward(s, S.cam_numpy(cam), do_depth=do_depth, drop_empty=drops_empty(P))
    out = dict(frame=fr, color=fr.color, invdepth=fr.invdepth)
    if grads is not None:
        g, gd = grads
        gr = O.backward(fr, s, g, gd if (do_depth or alt) else None)
        for k in GRADS:
            if k != "ddc" or alt:
                out[k] = gr[k]
    return out


def _check(gpu, ref, lists=True):
    fr = ref["frame"]
    np.testing.assert_array_equal(gpu["radii"], fr.radii)
    if lists:
        assert gpu["num_rendered"] == fr.R
        kept = binned(fr)
        assert gpu["misc"][0] == kept and gpu["misc"][1] == tile_counts(fr).max()
        # every tile's length, and the start of every non-empty tile: an empty tile's range is [0, 0) in the oracle
        # (the reference never writes it) and [s, s) at its place in the prefix sum on the GPU -- no entry either way
        c = tile_counts(fr)
        got = gpu["ranges"].astype(np.int64)
        np.testing.assert_array_equal(got[:, 1] - got[:, 0], c)
        np.testing.assert_array_equal(got[c > 0], fr.ranges[c > 0])
        np.testing.assert_array_equal(gpu["point_list"], fr.point_list[:kept])
        np.testing.assert_array_equal(gpu["n_contrib"], fr.n_contrib.astype(np.int32))
    for k in ("color", "invdepth"):
        if ref[k].size or gpu[k].size:
            mx, nbad, ok = image_check(gpu[k], ref[k])
            assert ok, f"{k} L-inf {mx} ({nbad} pixels over 1e-4)"
    for k in GRADS:
        if k in ref:
            assert_grad(k, gpu[k][..., :ref[k].shape[-1]], ref[k])


def _assert_one_tile(ref, n):
    """The cheap part of tests/test_dispatch_scenes_cpu.py on the test's own oracle frame."""
    c = tile_counts(ref["frame"])
    assert ref["frame"].R == n and (c > 0).sum() == 1 and c.max() == n


def _frame_info(sc, cam):
    """hlgs_frame_info of the scene's frame from the C ABI's one-call forward (buffer large enough to render)."""
    alt = bool(sc.get("alt"))
    _C = _front_end(alt)._C
    lib = L.load()
    W, H, P, deg = cam["W"], cam["H"], sc["means3D"].shape[0], sc["sh_degree"]
    t = lambda a: torch.tensor(np.ascontiguousarray(a), device=DEV)  # noqa: E731
    e = torch.empty(0, device=DEV)
    if alt:
        a, keep = _C._raster_args(cam["bg"], t(sc["means3D"]), e, t(sc["opacities"]), t(sc["scales"]),
                                  t(sc["rotations"]), 1.0, e, cam["viewmatrix"], cam["projmatrix"], cam["tanfovx"],
                                  cam["tanfovy"], H, W, t(sc["dc"]), t(sc["shs"]), deg, cam["campos"], False,
                                  sc["antialiasing"], False)[:2]
    else:
        a, keep = _C._raster_args(cam["bg"], e, e, e, e, t(sc["means3D"]), e, t(sc["opacities"]), t(sc["scales"]),
                                  t(sc["rotations"]), 1.0, e, cam["viewmatrix"], cam["projmatrix"], cam["tanfovx"],
                                  cam["tanfovy"], H, W, t(sc["shs"]), deg, cam["campos"], False, False)[:2]
    u8 = dict(dtype=torch.uint8, device=DEV)
    geom = torch.empty((lib.hlgs_geom_buffer_size(P),), **u8)
    img = torch.empty((lib.hlgs_image_buffer_size(W, H),), **u8)
    binning = torch.empty((lib.hlgs_binning_buffer_size(2 * P + 64),), **u8)
    radii = torch.empty((P,), dtype=torch.int32, device=DEV)
    color = torch.empty((3, H, W), device=DEV)
    invd = torch.empty((1, H, W), device=DEV)
    info = L.FrameInfo()
    L.check(lib.hlgs_rasterize_forward(C.byref(a), L.ptr(geom), L.ptr(img), L.ptr(radii), L.ptr(binning),
                                       binning.numel(), C.byref(info), L.ptr(color), L.ptr(invd), None, L.stream()))
    torch.cuda.synchronize()
    del keep
    return info


@contextlib.contextmanager
def _binning_hints(value):
    """Both front ends' binning-buffer hint for this device set to `value` (None: no hint) inside the block; what they
    held before is put back."""
    dev = torch.device("cuda", torch.cuda.current_device())
    hints = [_front_end(alt)._C._binning_hint for alt in (False, True)]
    before = [h.get(dev) for h in hints]
    try:
        for h in hints:
            h.pop(dev, None)
            if value is not None:
                h[dev] = value
        yield hints, dev
    finally:
        for h, b in zip(hints, before):
            h.pop(dev, None)
            if b is not None:
                h[dev] = b


def _one_tile_case(n, deg=0, alt=False, aa=True, do_depth=True, ties=False):
    sc, cam = one_tile_scene(n, seed=n, deg=deg, alt=alt, aa=aa)
    if ties:
        equal_depths(sc)
    g = S.upstream_grads(cam["W"], cam["H"], seed=1)
    ref = _ref(sc, cam, g, do_depth)
    _assert_one_tile(ref, n)
    return sc, cam, g, ref


# ---- per-tile list lengths -------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", SORT_N)
def test_sort_class_and_merge_parity_boundaries(n):
    """n entries on one tile at both sides of the wave-sort / block-sort / merge boundaries (1,024, 4,096) and of the
    merge passes' count and buffer parity (8,192, 16,384): lists, n_contrib, image and gradients."""
    sc, cam, g, ref = _one_tile_case(n)
    info = _frame_info(sc, cam)
    assert info.rendered == 1 and info.max_tile_count == n and info.num_binned == n
    _check(_gpu(sc, cam, g), ref)


@pytest.mark.parametrize("n", SORT_N_SMALL)
def test_sort_class_boundaries_with_plain_index_entries(n):
    """The same boundaries with plain-index point_list entries (the P >= 2^28 layout: no quadrant masks, nothing
    dropped)."""
    lib = L.load()
    try:
        lib.hlgs_set_entry_packing(0)
        assert lib.hlgs_point_list_entry_shift(n) == 0 and not drops_empty(n)
        sc, cam, g, ref = _one_tile_case(n)
        info = _frame_info(sc, cam)
        assert info.entry_shift == 0 and info.max_tile_count == n
        _check(_gpu(sc, cam, g), ref)
    finally:
        lib.hlgs_set_entry_packing(1)
    assert lib.hlgs_point_list_entry_shift(n) != 0


@pytest.mark.parametrize("aa", [True, False])
@pytest.mark.parametrize("n", SORT_N_SMALL)
def test_sort_class_boundaries_alt(n, aa):
    sc, cam, g, ref = _one_tile_case(n, deg=1, alt=True, aa=aa)
    info = _frame_info(sc, cam)
    assert info.rendered == 1 and info.max_tile_count == n
    _check(_gpu(sc, cam, g), ref)


@pytest.mark.parametrize("do_depth", [True, False])
@pytest.mark.parametrize("deg", [0, 3])
@pytest.mark.parametrize("n", CHUNK_N)
def test_backward_chunk_and_blend_batch_boundaries(n, deg, do_depth):
    """Lists of 63 / 64 / 65 entries (one 64-splat batch or two) and at both sides of bwd_chunk_len's steps (192 | 193:
    one chunk or two, 384 | 385: two or three, 576 | 577: chunks of 192 or longer); some pixel stays live through the
    whole list (n_contrib.max() == n), so every chunk of the backward has work."""
    sc, cam, g, ref = _one_tile_case(n, deg=deg, do_depth=do_depth)
    assert ref["frame"].n_contrib.max() == n
    gpu = _gpu(sc, cam, g, do_depth=do_depth)
    assert gpu["misc"][1] == n
    _check(gpu, ref)


@pytest.mark.parametrize("n", CHUNK_N_ALT)
def test_backward_chunk_boundaries_alt(n):
    sc, cam, g, ref = _one_tile_case(n, deg=3, alt=True)
    assert ref["frame"].n_contrib.max() == n
    gpu = _gpu(sc, cam, g)
    assert gpu["misc"][1] == n
    _check(gpu, ref)


@pytest.mark.parametrize("n", TIE_N)
def test_equal_depths_stay_in_index_order(n):
    """Every sort key ties (helpers.equal_depths): the list is 0..n-1 in order across the wave-sort | block-sort
    boundary (1,025) and across the block sort's runs and the merge (4,097)."""
    sc, cam, g, ref = _one_tile_case(n, ties=True)
    assert np.unique(ref["frame"].depths).size == 1
    gpu = _gpu(sc, cam, g)
    np.testing.assert_array_equal(gpu["point_list"], np.arange(n, dtype=np.uint32))
    _check(gpu, ref)


# ---- Gaussian-count thresholds ---------------------------------------------------------------------------------

def _sparse_case(P, deg, bg, nb):
    assert bin_gauss(P) == bg and -(-P // bg) == nb  # the side of the thresholds this P is on
    W, H = SPARSE_WH
    sc, cam, _ = sparse_scene(P, seed=P % 1000, W=W, H=H, deg=deg)
    g = S.upstream_grads(W, H, seed=2)
    ref = _ref(sc, cam, g)
    fr = ref["frame"]
    assert fr.R > 0 and fr.radii[P - 1] > 0 and np.unique(np.nonzero(fr.radii > 0)[0] // bg).size > nb // 2
    return sc, cam, g, ref


@pytest.mark.parametrize("P,deg,bg,nb", SPARSE)
def test_gaussian_count_thresholds_default_plan(P, deg, bg, nb):
    """The fused plan (k_tile_offsets_plan) at both sides of nb = 256 | 257 (<8> | <24>) with 1,024- and 4,096-Gaussian
    blocks, of bin_gauss's switch (786,432 | 786,433: nb 768 of 1,024 | 193 of 4,096) and of nb = 768 | 769 (<24>'s
    registers | its loop): lists, n_contrib, image and gradients.  9 look-back blocks (260 tiles)."""
    sc, cam, g, ref = _sparse_case(P, deg, bg, nb)
    gpu = _gpu(sc, cam, g)
    assert gpu["misc"][K_MISC_FAIL] == 0
    _check(gpu, ref)


@pytest.mark.parametrize("P,deg,bg,nb", [c for c in SPARSE if c[0] in (262145, 786432, 786433, 1048577)])
def test_gaussian_count_thresholds_forced_replan(P, deg, bg, nb):
    """hlgs_set_plan_polls(0): every look-back block but the first times out, the frame is planned again by
    k_count_tiles + k_tile_offsets + k_plan, and must match the oracle exactly: k_tile_offsets<24> with 1,024-Gaussian
    blocks (nb 257, 768) and with 4,096-Gaussian blocks (nb 257), k_tile_offsets<8> with 4,096-Gaussian blocks (nb 193).
    That the re-plan ran: the image buffer's misc[5] (kMiscFail) is still set after the frame -- a timed-out block sets
    it, and only the count kernel of a fused plan clears it, which the re-plan's is not.  The next frame, with the
    default bound, leaves it 0."""
    lib = L.load()
    sc, cam, g, ref = _sparse_case(P, deg, bg, nb)
    assert (bg, nb) in ((1024, 257), (1024, 768), (4096, 193), (4096, 257))
    try:
        lib.hlgs_set_plan_polls(0)
        gpu = _gpu(sc, cam, g)
    finally:
        lib.hlgs_set_plan_polls(1 << 20)
    assert gpu["misc"][K_MISC_FAIL] != 0
    _check(gpu, ref)
    again = _gpu(sc, cam, g)
    assert again["misc"][K_MISC_FAIL] == 0
    _check(again, ref)
    for k in LISTS + GRADS[:-1] + ("color", "invdepth"):
        np.testing.assert_array_equal(gpu[k], again[k])


@pytest.mark.parametrize("P", [1, 1024, 1025, 7 * 1024 + 1, 8 * 1024, 9 * 1024 - 1, 31 * 1024 + 5, 33 * 1024])
def test_hist_rows_small_block_counts(P):
    """nb = 1, 1, 2, 8 (one row per XCD), 8, 9, 32 (one row per thread group; the last block holds 5 Gaussians) and 33:
    HistRows steps the histogram rows with nb / 8 and nb % 8, and a thread's run is ceil(nb / 32) rows."""
    W, H = 96, 80
    cam = S.make_camera(W, H)
    sc = S.make_gaussians(P, 1, cam, seed=P)
    ref = _ref(sc, cam)
    assert ref["frame"].R > 0
    _check(_gpu(sc, cam), ref)


# ---- state carried from frame to frame -----------------------------------------------------------------------------

@pytest.mark.parametrize("small_buffers", [False, True])
def test_frame_order_does_not_matter(small_buffers):
    """S, S, M, M, L, L, S, L, M, S (longest list 600 / 2,000 / 5,000: wave sort, block sort, merge) in one thread: the
    speculative render queues the sorts the previous frame needed (Readback::last_maxc), so the sequence takes all nine
    ordered transitions -- the queued block sort kept (M after M / L), run over short lists (S after M / L), missing
    (M / L after S) or not enough (L after M / L).  Every frame against the oracle; frames of one scene bitwise equal.
    small_buffers: the front end's binning hint is 1 byte before the first M and before the L after S, so those
    frames are rendered by the second call (hlgs_rasterize_forward_render); the buffer the first M leaves (2,000
    entries + 15%) is the one the first L outgrows, whose speculative render is queued and exits on capacity."""
    scenes = {}
    for k, n in zip("SML", ORDER_N):
        sc, cam = one_tile_scene(n, seed=n, deg=1)
        g = S.upstream_grads(cam["W"], cam["H"], seed=3)
        ref = _ref(sc, cam, g)
        _assert_one_tile(ref, n)
        scenes[k] = (sc, cam, g, ref, n)
    first = {}
    with _binning_hints(1 << 26) as (hints, dev):
        for i, k in enumerate("SSMMLLSLMS"):
            if small_buffers and i in (2, 7):
                hints[0][dev] = 1
            sc, cam, g, ref, n = scenes[k]
            gpu = _gpu(sc, cam, g)
            assert gpu["misc"][1] == n, (i, k)
            _check(gpu, ref)
            if k in first:
                for key in LISTS + GRADS[:-1] + ("color", "invdepth", "radii"):
                    np.testing.assert_array_equal(gpu[key], first[k][key], err_msg=f"frame {i} ({k}): {key}")
            else:
                first[k] = gpu


# ---- the caller's stream -------------------------------------------------------------------------------------------

class _Replay:
    """The stream test's `up`: the first pass (default stream) uploads every input and keeps the device tensors in call
    order; the second pass (side stream) hands out, in the same order, copies made on the current stream that depend
    on a long kernel queued there first -- t * one, with one = (A @ A)[0, 0] + 1 for a zero matrix A -- so that no
    host copy waits for the stream and every kernel launched meanwhile is queued behind unfinished work.  A launch that
    went to another stream would read inputs not yet written."""

    def __init__(self):
        self.kept, self.pos, self.side = [], 0, False
        self.a = torch.zeros((8192, 8192), device=DEV)
        self.ev = self.one = None

    def busy_one(self):
        if self.ev is None or self.ev.query():  # keep the stream busy without piling matmuls up
            self.one = (self.a @ self.a)[0, 0] + 1.0
            self.ev = torch.cuda.Event()
            self.ev.record()
        return self.one

    def __call__(self, a):
        if not self.side:
            self.kept.append(_upload(a))
            return self.kept[-1].clone()
        t = self.kept[self.pos]
        self.pos += 1
        return t * self.busy_one().to(t.dtype)


def _all_bindings(up):
    """Forward and backward of every binding that launches on torch's current stream -> list of (name, host array)."""
    import gaussian_hierarchy as GH
    from fused_ssim import fused_ssim
    from hlgs_core.activations import activate
    res = []
    cam = S.make_camera(128, 96)
    g = S.upstream_grads(128, 96, seed=1)
    for alt in (False, True):
        sc = S.make_gaussians(2000, 3, cam, seed=5)
        if alt:
            sc.update(dc=np.ascontiguousarray(sc["shs"][:, :1]), shs=np.ascontiguousarray(sc["shs"][:, 1:]), alt=True,
                      antialiasing=True)
        r = _gpu(sc, cam, g, up=up)
        res += [(f"raster alt={alt} {k}", v) for k, v in sorted(r.items()) if isinstance(v, np.ndarray)]
    # S then L of test_frame_order_does_not_matter: the queued wave sort is not enough, the frame is rendered again
    for n in (ORDER_N[0], ORDER_N[2]):
        sc, c1 = one_tile_scene(n, seed=n, deg=1)
        r = _gpu(sc, c1, S.upstream_grads(64, 64, seed=3), up=up)
        assert r["misc"][1] == n
        res += [(f"one tile {n} {k}", v) for k, v in sorted(r.items()) if isinstance(v, np.ndarray)]
    rng = np.random.default_rng(11)
    a = rng.uniform(0, 1, (2, 3, 77, 131)).astype(np.float32)
    b = np.clip(a + rng.normal(0, 0.1, a.shape), 0, 1).astype(np.float32)
    x = up(a).detach().requires_grad_(True)
    s = fused_ssim(x, up(b))
    s.backward()
    res += [("ssim", s.detach().cpu().numpy()), ("ssim grad", x.grad.cpu().numpy())]
    raw = [up(rng.normal(size=(1000, w)).astype(np.float32)).detach().requires_grad_(True) for w in (1, 3, 4)]
    act = activate(*raw)
    torch.autograd.backward(act, [up(rng.normal(size=tuple(t.shape)).astype(np.float32)) for t in act])
    res += [(f"activate {i}", t.detach().cpu().numpy()) for i, t in enumerate(act)]
    res += [(f"activate grad {i}", t.grad.cpu().numpy()) for i, t in enumerate(raw)]
    h = S.make_dynamic_hierarchy(S.make_gaussians(800, 3, cam, seed=0), seed=0)
    N = h["nodes"].shape[0]
    vp, vd = np.zeros(3, np.float32), np.array([0, 0, 1], np.float32)
    nodes, pos, scl = up(h["nodes"]), up(h["means3D"]), up(h["scales"])
    ri, pi, ni = (torch.zeros(N, dtype=torch.int32, device=DEV) for _ in range(3))
    n = GH.expand_to_size_dynamic(nodes, pos, scl, 0.002, up(vp), torch.tensor(vd), ri, pi, ni)
    assert 0 < n < N
    ts = torch.zeros(N, device=DEV)
    kids = torch.zeros(N, dtype=torch.int32, device=DEV)
    GH.get_interpolation_weights_dynamic(ni[:n], 0.002, nodes, pos, scl, torch.tensor(vp), torch.tensor(vd), ts, kids)
    res += [("expand " + k, t[:n].cpu().numpy()) for k, t in (("ri", ri), ("pi", pi), ("ni", ni), ("ts", ts),
                                                              ("kids", kids))]
    leaves = [up(h[k]).detach().requires_grad_(True) for k in ("means3D", "scales", "rotations", "opacities", "shs")]
    outs = GH.interpolate_lod(*leaves, ri[:n], pi, ts, 0)
    torch.autograd.backward(outs, [up(rng.normal(size=tuple(t.shape)).astype(np.float32)) for t in outs])
    res += [(f"lerp {i}", t.detach().cpu().numpy()) for i, t in enumerate(outs)]
    res += [(f"lerp grad {i}", t.grad.cpu().numpy()) for i, t in enumerate(leaves)]
    return res


def test_bindings_on_a_side_stream_match_the_default_stream():
    """Both rasterizers, fused_ssim, activate, expand_to_size_dynamic + get_interpolation_weights_dynamic and
    interpolate_lod, forward and backward, on a non-default stream behind a long kernel (see _Replay), inputs made on
    that stream: bit for bit what the same calls give on the default stream.  The forward's pinned-word polling and
    hipStreamQuery then run against that stream, and a launch on the null stream by mistake would not be ordered behind
    the inputs."""
    up = _Replay()
    with _binning_hints(1 << 26):
        want = _all_bindings(up)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        assert side != torch.cuda.default_stream()
        up.side = True
        with torch.cuda.stream(side):
            got = _all_bindings(up)
            side.synchronize()
        torch.cuda.synchronize()
    assert up.pos == len(up.kept) and [k for k, _ in got] == [k for k, _ in want]
    for (k, a), (_, b) in zip(got, want):
        np.testing.assert_array_equal(a, b, err_msg=k)
