#!/usr/bin/env python3
"""Measurements of the rows around the rasterizer hot path, on one GPU:

  lod       config #3: a synthetic binary hierarchy over config #2's 1M leaves (~2M nodes), cut with
            expand_to_size_dynamic at tau = 2 (6 + 0.5) tanfovx / (0.5 W) (render_hierarchy.py:56), interpolation
            weights, the render_post lerp (interpolate_lod), then rasterizer forward + backward at 1080p and the
            lerp's backward: each stage separately and the whole step inclusive.
  alt       the alt rasterizer (train_post.py's default) on config #2: forward + backward Mpix/s.
  loss      photometric_loss (L1 + D-SSIM + masked inverse-depth L1) forward + backward on a 1080p view.
  loss_exp  the same loss for a view with a trained (3, 4) exposure and an alpha mask (clamp_image=True), gradients to
            the image and the exposure: the fused call beside the torch composition it replaces, alternated, three
            runs each.
  act_reg   the parameter activations of --P resident rows with the MCMC opacity and scale regularisers
            (train_post.py:565-576), forward + backward: activate() alone, activate() plus the torch expression of the
            two terms, and activate_regularized, alternated, three runs each.
  adam      SparseGaussianAdam.step over 1M Gaussians (59 floats each, six parameter groups), half visible.
  morton    get_morton_indices over the hierarchy's nodes.
  knn       simple_knn.distCUDA2 (create_from_pcd's initial scales) at 250k, 1M and 4M points on a uniform cube and
            on a Gaussian cloud with a 10% skybox shell at 10x its radius, the scenes alternated from round to round;
            beside them the all-pairs torch restatement (tests/knn_ref.py) at 250k, timed once.
  hier_build  hlgs_core.hierarchy.build_dynamic_hierarchy (the offline GaussianHierarchyCreator on the GPU) over
            250k, 1M and 4M synthetic leaves with 48 SH floats: the whole build and every stage on its own (event
            times; the stages are then one call each); beside them the wall time of the recursive numpy restatement
            (tests/hier_build_ref.py) at 20,000 leaves and of synthetic.make_dynamic_hierarchy at 1M.
  hier_merge  hlgs_core.hierarchy.merge_dynamic_hierarchies (the offline GaussianHierarchyMerger on the GPU) over K = 4
            chunks of 250k, 1M and 4M rows each (48 SH floats; leaves uniform in a cube of half-side 3.2 around
            centres 4 apart, the trees built by build_dynamic_hierarchy): the whole call, read-backs and allocation
            included (median of 5, host clock), every stage by events, and the bytes the scatter must move (kept rows
            x row bytes, read + write) over its time as a fraction of HBM; beside them the wall time of the recursive
            numpy restatement (tests/hier_merge_ref.py) at 20,011 leaves per chunk.
  spt_nary  the n-ary SPT path on merge_dynamic_hierarchies' output for K = 4 chunks of 250k rows (hier_merge's
            recipe, 3 SH floats) beside the binary path on make_dynamic_hierarchy of the same row count:
            build_hierarchical_spt_device, and one view's coarse cut of the resulting upper tree by the flat cut and
            by the level walk (host clock around a device synchronise, median of 5 after a warm-up); the volume is
            the one that 0.5 % of each hierarchy's inner nodes exceed.  The same again with the volume at the first
            quartile, where no SPT is kept and the whole hierarchy is the upper tree; and the n-ary level walk over
            a root with 2, 300 and 3,000 leaf children (the cost of a round of its rank loop) and over a chain of
            299 one-child nodes.
  stream    train_post.py's SPT cache over the same hierarchy: SPT construction (host code), then a camera path
            of views through SPTCache.step (coarse cut, cache bookkeeping, SPT cut, write-back and load of the
            six parameters and twelve Adam moments to and from pinned host storage) and the dense Adam step of
            the resident set; per-stage times and the host-link bytes moved per view.

Times are medians of CUDA-event spans on torch's current stream (the library launches there).  Inputs are
synthetic (seeded) and resident on the device.  Prints one JSON object.
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hierarchical-lod-gaussians_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from hlgs_core import synthetic as S  # noqa: E402

DEV = "cuda"
HBM = 8000.0


def timed(fn, iters=20, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def settings(cam, deg, do_depth=True, alt=False):
    e_i = torch.empty(0, dtype=torch.int32, device=DEV)
    e_f = torch.empty(0, dtype=torch.float32, device=DEV)
    common = dict(image_height=cam["H"], image_width=cam["W"], tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"],
                  bg=torch.zeros(3, device=DEV), scale_modifier=1.0, viewmatrix=cam["viewmatrix"].to(DEV),
                  projmatrix=cam["projmatrix"].to(DEV), sh_degree=deg, campos=cam["campos"].to(DEV),
                  prefiltered=False, debug=False)
    if alt:
        from alt_gaussian_rasterization import GaussianRasterizationSettings
        return GaussianRasterizationSettings(antialiasing=True, **common)
    from diff_gaussian_rasterization import GaussianRasterizationSettings
    return GaussianRasterizationSettings(render_indices=e_i, parent_indices=e_i, interpolation_weights=e_f,
                                         num_node_kids=e_i, do_depth=do_depth, **common)


def bench_alt(P, W, H, deg):
    from alt_gaussian_rasterization import GaussianRasterizer
    cam = S.make_camera(W, H)
    h = S.make_gaussians(P, deg, cam, seed=0)
    t = lambda a: torch.tensor(np.ascontiguousarray(a), device=DEV, requires_grad=True)  # noqa: E731
    m, sc, r, o = t(h["means3D"]), t(h["scales"]), t(h["rotations"]), t(h["opacities"])
    dc, rest = t(h["shs"][:, :1]), t(h["shs"][:, 1:])
    g_np, gd_np = S.upstream_grads(W, H, seed=1)
    g, gd = torch.tensor(g_np, device=DEV), torch.tensor(gd_np, device=DEV)
    rast = GaussianRasterizer(settings(cam, deg, alt=True))

    def step():
        m2 = torch.zeros_like(m, requires_grad=True)
        c, _, inv = rast(means3D=m, means2D=m2, opacities=o, dc=dc, shs=rest, scales=sc, rotations=r)
        torch.autograd.backward([c, inv], [g, gd])

    ms = timed(step)
    return dict(workload=f"alt rasterizer, {P} Gaussians, SH deg {deg}, {W}x{H}, fwd+bwd (antialiasing)",
                ms=round(ms, 4), Mpix_s=round(W * H / ms / 1e3, 1))


def bench_loss(W, H):
    from hlgs_core import loss
    rng = np.random.default_rng(0)
    img = torch.tensor(rng.uniform(0, 1, (3, H, W)).astype(np.float32), device=DEV, requires_grad=True)
    gt = torch.tensor(rng.uniform(0, 1, (3, H, W)).astype(np.float32), device=DEV)
    inv = torch.tensor(rng.uniform(0.05, 0.5, (1, H, W)).astype(np.float32), device=DEV, requires_grad=True)
    mono = torch.tensor(rng.uniform(0.05, 0.5, (1, H, W)).astype(np.float32), device=DEV)
    mask = torch.ones((1, H, W), device=DEV)

    def step():
        tot = loss.photometric_loss(img, gt, 0.2, inv, mono, mask, 0.5)[0]
        tot.backward()

    ms = timed(step)
    N = W * H
    # algorithmic HBM bytes: fwd reads both images (24 B/px) and writes 3 derivative maps per channel (36 B/px);
    # bwd reads the maps and both images (60 B/px) and writes the image gradient (12 B/px); depth term
    # reads 12 B/px twice and writes 4 B/px
    alg = N * (24 + 36 + 60 + 12) + N * (12 + 12 + 4)
    return dict(workload=f"photometric loss (L1 + D-SSIM + depth L1), 3x{H}x{W}, fwd+bwd", ms=round(ms, 4),
                alg_GBs=round(alg / (ms * 1e-3) / 1e9, 1), hbm_frac=round(alg / (ms * 1e-3) / 1e9 / HBM, 3))


def bench_loss_exp(W, H, legs=("fused", "composed"), runs=3):
    """The loss of a view with a trained exposure and an alpha mask, forward + backward to the image and the exposure:
    `fused` is photometric_loss(..., clamp_image=True, exposure=E, alpha_mask=m); `composed` is what a caller wrote
    before it, in the same process -- the reference's torch expression (gaussian_renderer/__init__.py:139-141),
    .clamp(0, 1), * mask, then the plain photometric_loss.  Each run is timed()'s median after its own untimed settle
    steps; the legs alternate, `runs` runs each."""
    from hlgs_core import loss
    rng = np.random.default_rng(0)
    img = torch.tensor(rng.uniform(-0.3, 1.3, (3, H, W)).astype(np.float32), device=DEV, requires_grad=True)
    mask = torch.tensor(rng.uniform(0, 1, (1, H, W)).astype(np.float32), device=DEV)
    gt = torch.tensor(rng.uniform(0, 1, (3, H, W)).astype(np.float32), device=DEV) * mask
    E0 = np.eye(3, 4) + np.concatenate([0.15 * rng.standard_normal((3, 3)), 0.05 * rng.standard_normal((3, 1))], 1)
    E = torch.tensor(E0.astype(np.float32), device=DEV, requires_grad=True)

    def fused():
        img.grad = E.grad = None
        loss.photometric_loss(img, gt, 0.2, clamp_image=True, exposure=E, alpha_mask=mask)[0].backward()

    def composed():
        img.grad = E.grad = None
        x = torch.matmul(img.permute(1, 2, 0), E[:3, :3]).permute(2, 0, 1) + E[:3, 3, None, None]
        loss.photometric_loss(x.clamp(0, 1) * mask, gt, 0.2)[0].backward()

    fns = dict(fused=fused, composed=composed)
    ms = {k: [] for k in legs}
    for _ in range(runs):
        for k in legs:
            ms[k].append(round(timed(fns[k]), 4))
    out = dict(workload=f"photometric loss with exposure (3, 4), clamp and alpha mask, 3x{H}x{W}, fwd+bwd",
               runs_ms=ms, min_ms={k: min(v) for k, v in ms.items()}, max_ms={k: max(v) for k, v in ms.items()})
    if "fused" in legs:
        N = W * H
        # algorithmic HBM bytes of the fused leg: fwd reads image, gt and mask (28 B/px) and writes the maps (36 B/px);
        # bwd reads the maps, image, gt and mask (64 B/px) and writes the image gradient (12 B/px)
        alg = N * (28 + 36 + 64 + 12)
        out["fused_alg_GBs"] = round(alg / (min(ms["fused"]) * 1e-3) / 1e9, 1)
    return out


def bench_act_reg(P, runs=3):
    """The activations of P resident rows with the MCMC regularisers (train_post.py:565-576), forward + backward with
    upstream gradients on the three activated outputs and loss = 0.01 opacity_loss + 0.02 scaling_loss: `activate` is
    activate() alone (no regularisers), `composed` is activate() plus the torch expression of the two terms, which is
    what a caller wrote before activate_regularized, and `fused` is activate_regularized.  Each run is timed()'s
    median; the legs alternate, `runs` runs each.  fused_le_composed is the condition the fused call has to meet;
    fused_minus_activate_ms is what the regularisers cost."""
    from hlgs_core.activations import activate, activate_regularized
    from hlgs_core.mcmc import add_regularizers
    g = torch.Generator(device=DEV).manual_seed(0)
    op = (torch.randn((P, 1), device=DEV, generator=g) * 4).requires_grad_(True)
    sc = (torch.randn((P, 3), device=DEV, generator=g) * 2 - 4).requires_grad_(True)
    rot = torch.randn((P, 4), device=DEV, generator=g).requires_grad_(True)
    ups = [torch.randn(s, device=DEV, generator=g) for s in ((P, 1), (P, 3), (P, 4))]

    def clear():
        op.grad = sc.grad = rot.grad = None

    def plain():
        clear()
        torch.autograd.backward(activate(op, sc, rot), ups)

    def composed():
        clear()
        o, s, r = activate(op, sc, rot)
        loss = add_regularizers(0.0, torch.sum(torch.abs(o)) / P, torch.sum(torch.abs(s)) / P, 0.01, 0.02)
        torch.autograd.backward([o, s, r, loss], ups + [None])

    def fused():
        clear()
        o, s, r, ol, sl = activate_regularized(op, sc, rot)
        torch.autograd.backward([o, s, r, add_regularizers(0.0, ol, sl, 0.01, 0.02)], ups + [None])

    fns = dict(activate=plain, composed=composed, fused=fused)
    ms = {k: [] for k in fns}
    for _ in range(runs):
        for k, fn in fns.items():
            ms[k].append(round(timed(fn, iters=50, warmup=5), 4))
    med = {k: round(float(np.median(v)), 4) for k, v in ms.items()}
    alg = P * 4 * (8 + 8 + 8 + 8 + 8)  # fwd: 8 floats read, 8 written; bwd: 8 + 8 read (rows, upstream), 8 written
    return dict(workload=f"activations of {P} rows with the opacity and scale regularisers, fwd+bwd", runs_ms=ms,
                median_ms=med, fused_le_composed=bool(med["fused"] <= med["composed"]),
                fused_minus_activate_ms=round(med["fused"] - med["activate"], 4),
                fused_alg_GBs=round(alg / (med["fused"] * 1e-3) / 1e9, 1))


def bench_adam(P):
    from alt_gaussian_rasterization import SparseGaussianAdam
    widths = dict(xyz=3, f_dc=3, f_rest=45, opacity=1, scaling=3, rotation=4)
    params = {k: torch.nn.Parameter(torch.randn(P, w, device=DEV)) for k, w in widths.items()}
    opt = SparseGaussianAdam([{"params": [p], "lr": 1e-3, "name": k} for k, p in params.items()], lr=0.0, eps=1e-15)
    for p in params.values():
        p.grad = torch.randn_like(p)
    vis = torch.rand(P, device=DEV) < 0.5
    ms = timed(lambda: opt.step(vis, P))
    alg = 0.5 * P * 59 * 28 + P  # visible elements: 16 B read + 12 B written; one visibility byte per Gaussian
    return dict(workload=f"SparseGaussianAdam.step, {P} Gaussians x 59 floats, 50% visible", ms=round(ms, 4),
                alg_GBs=round(alg / (ms * 1e-3) / 1e9, 1), hbm_frac=round(alg / (ms * 1e-3) / 1e9 / HBM, 3))


def bench_lod(P, W, H, deg):
    import gaussian_hierarchy as GH
    from diff_gaussian_rasterization import GaussianRasterizer
    cam = S.make_camera(W, H)
    t0 = time.perf_counter()
    hier = S.make_dynamic_hierarchy(S.make_gaussians(P, deg, cam, seed=0), seed=0)
    build_s = time.perf_counter() - t0
    N = hier["nodes"].shape[0]
    d = lambda a, **kw: torch.tensor(np.ascontiguousarray(a), device=DEV, **kw)  # noqa: E731
    nodes, xyz, scales = d(hier["nodes"]), d(hier["means3D"], requires_grad=True), d(hier["scales"], requires_grad=True)
    rots, opac, shs = (d(hier["rotations"], requires_grad=True), d(hier["opacities"], requires_grad=True),
                       d(hier["shs"], requires_grad=True))
    tau = (2 * (6 + 0.5)) * cam["tanfovx"] / (0.5 * W)
    vp = cam["campos"].to(DEV)
    vd = torch.tensor([0.0, 0.0, 1.0])
    ri = torch.zeros(N, dtype=torch.int32, device=DEV)
    pi = torch.zeros(N, dtype=torch.int32, device=DEV)
    ni = torch.zeros(N, dtype=torch.int32, device=DEV)
    ts = torch.zeros(N, device=DEV)
    kids = torch.zeros(N, dtype=torch.int32, device=DEV)
    rast = GaussianRasterizer(settings(cam, deg, do_depth=True))
    g_np, gd_np = S.upstream_grads(W, H, seed=1)
    g, gd = torch.tensor(g_np, device=DEV), torch.tensor(gd_np, device=DEV)
    state = {}

    def cut():
        state["n"] = GH.expand_to_size_dynamic(nodes, xyz.detach(), scales.detach(), tau, vp, vd, ri, pi, ni)

    def weights():
        n = state["n"]
        GH.get_interpolation_weights_dynamic(ni[:n], tau, nodes, xyz.detach(), scales.detach(), vp.cpu(), vd, ts, kids)

    def lerp():
        n = state["n"]
        state["outs"] = GH.interpolate_lod(xyz, scales, rots, opac, shs, ri[:n], pi, ts, 0)

    def raster():
        m, s_, r_, o_, sh_ = state["outs"]
        m2 = torch.zeros_like(m, requires_grad=True)
        c, _, inv = rast(means3D=m, means2D=m2, opacities=o_, shs=sh_, scales=s_, rotations=r_)
        state["graph"] = (c, inv)

    def backward():
        c, inv = state["graph"]
        torch.autograd.backward([c, inv], [g, gd])
        for p in (xyz, scales, rots, opac, shs):
            p.grad = None

    def full():
        cut(); weights(); lerp(); raster(); backward()  # noqa: E702

    full()
    stages = {}
    for name, fn in (("expand_to_size_dynamic", cut), ("get_interpolation_weights_dynamic", weights),
                     ("interpolate_lod_fwd", lerp)):
        stages[name] = round(timed(fn), 4)
    stages["rasterizer_fwd"] = round(timed(raster), 4)

    def raster_bwd():
        lerp(); raster()  # noqa: E702
        backward()

    stages["rasterizer_bwd+lerp_bwd"] = round(timed(raster_bwd) - stages["interpolate_lod_fwd"] -
                                              stages["rasterizer_fwd"], 4)
    incl = timed(full)
    n = state["n"]
    return dict(workload=f"config #3: synthetic binary hierarchy over {P} leaves ({N} nodes), SH deg {deg}, {W}x{H}, "
                         f"tau={tau:.3e}, cut -> weights -> lerp -> rasterize fwd+bwd -> lerp bwd",
                nodes=N, selected=n, hierarchy_build_s=round(build_s, 1), stages_ms=stages,
                inclusive_ms=round(incl, 4), lod_cut_and_interp_ms=round(sum(stages[k] for k in (
                    "expand_to_size_dynamic", "get_interpolation_weights_dynamic", "interpolate_lod_fwd")), 4),
                Mpix_s=round(W * H / incl / 1e3, 1)), (xyz.detach(), N)


def bench_morton(xyz):
    import gaussian_hierarchy as GH
    codes = torch.zeros(xyz.shape[0], dtype=torch.int64, device=DEV)
    mn, mx = xyz.min(0)[0], xyz.max(0)[0]
    ms = timed(lambda: GH.get_morton_indices(xyz, mn, mx, codes))
    alg = xyz.shape[0] * (12 + 8)
    return dict(workload=f"get_morton_indices, {xyz.shape[0]} points", ms=round(ms, 4),
                alg_GBs=round(alg / (ms * 1e-3) / 1e9, 1))


def knn_scene(name, P, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    if name == "cube":
        return torch.rand((P, 3), device=DEV, generator=g)
    S_ = P // 10  # cloud + skybox shell, as create_from_pcd makes it (scene/gaussian_model.py:829-838)
    cloud = torch.randn((P - S_, 3), device=DEV, generator=g)
    mean = cloud.mean(0)
    radius = torch.linalg.norm(cloud.max(0)[0] - mean)
    theta = 2.0 * math.pi * torch.rand(S_, device=DEV, generator=g)
    phi = torch.arccos(1.0 - 1.4 * torch.rand(S_, device=DEV, generator=g))
    shell = radius * 10 * torch.stack((torch.cos(theta) * torch.sin(phi), torch.sin(theta) * torch.sin(phi),
                                       torch.cos(phi)), 1) + mean
    return torch.cat((shell, cloud)).contiguous()


def bench_knn(sizes=(250_000, 1_000_000, 4_000_000), rounds=5, calls=4, restatement_P=250_000):
    from simple_knn._C import distCUDA2, plan
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from knn_ref import knn_ref
    names = ("cube", "cloud_skybox")
    out = dict(workload="simple_knn.distCUDA2: mean squared distance to the 3 nearest other points", sizes={})
    for P in sizes:
        pts = {n: knn_scene(n, P) for n in names}
        for n in names:  # settle: code objects, allocator
            for _ in range(3):
                distCUDA2(pts[n])
        torch.cuda.synchronize()
        ms = {n: [] for n in names}
        for _ in range(rounds):  # alternate the scenes so that drift of the shared host hits both alike
            for n in names:
                ms[n].append(timed(lambda: distCUDA2(pts[n]), iters=calls, warmup=1))
        out["sizes"][str(P)] = dict(plan=plan(P), **{n: dict(ms=round(float(np.median(ms[n])), 4),
                                                             ms_min=round(min(ms[n]), 4), ms_max=round(max(ms[n]), 4),
                                                             ns_per_point=round(float(np.median(ms[n])) * 1e6 / P, 3))
                                                     for n in names})
        if P == restatement_P:
            knn_ref(pts["cube"][:4096], DEV)  # settle
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ref = knn_ref(pts["cube"], DEV)
            torch.cuda.synchronize()
            out["restatement"] = dict(workload=f"all-pairs torch restatement, cube, {P} points, one run",
                                      ms=round((time.perf_counter() - t0) * 1e3, 1),
                                      bitwise_equal=bool(torch.equal(ref.view(torch.int32),
                                                                     distCUDA2(pts["cube"]).view(torch.int32))))
        del pts
    return out


def bench_hier_build(sizes=(250_000, 1_000_000, 4_000_000), restatement_P=20_000, numpy_builder_P=1_000_000):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import hier_build_ref as HR
    from hlgs_core import hierarchy as H
    cam = S.make_camera(1920, 1080)
    out = dict(lds_cap=H.LDS_CAP)

    def inputs(P):
        g = S.make_gaussians(P, 3, cam, seed=0)
        return g, [torch.tensor(g[k], device=DEV) for k in ("means3D", "shs", "opacities", "scales", "rotations")]

    for P in sizes:
        print(f"hier_build: {P} leaves", file=sys.stderr, flush=True)
        _, dev = inputs(P)
        whole = timed(lambda: H.build_dynamic_hierarchy(*dev), iters=5, warmup=1)
        stages = []
        for _ in range(3):
            ms = {}
            H.build_dynamic_hierarchy(*dev, stage_ms=ms)
            stages.append(ms)
        out[str(P)] = dict(workload=f"{P} leaves, 48 SH floats, {2 * P - 1} rows out", build_ms=round(whole, 3),
                           leaves_per_s=round(P / (whole * 1e-3)),
                           stage_ms={k: round(float(np.median([m[k] for m in stages])), 3) for k in H.STAGES})
        del dev
    g, dev = inputs(restatement_P)
    sc = dict(xyz=g["means3D"], shs=g["shs"].reshape(restatement_P, -1), opacity=g["opacities"].reshape(-1),
              scales=g["scales"], rotations=g["rotations"])
    t0 = time.perf_counter()
    ref = HR.build_ref(sc, np.float32)
    ref_s = time.perf_counter() - t0
    nodes = H.build_dynamic_hierarchy(*dev)[5].cpu().numpy()
    out["restatement"] = dict(workload=f"recursive numpy restatement, float32, {restatement_P} leaves, one run",
                              s=round(ref_s, 2), gpu_ms=round(timed(lambda: H.build_dynamic_hierarchy(*dev), 5, 1), 3),
                              nodes_equal=bool((nodes == ref["nodes"]).all()))
    g = S.make_gaussians(numpy_builder_P, 3, cam, seed=0)
    t0 = time.perf_counter()
    S.make_dynamic_hierarchy(g, seed=0)
    out["make_dynamic_hierarchy"] = dict(workload=f"synthetic.make_dynamic_hierarchy (numpy, Morton pairs), "
                                                  f"{numpy_builder_P} leaves, one run",
                                         s=round(time.perf_counter() - t0, 2))
    return out


def bench_hier_merge(sizes=(250_000, 1_000_000, 4_000_000), K=4, shf=48, restatement_L=20_011):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import hier_merge_ref as MR
    from hlgs_core import hierarchy as H
    cen = MR.centers_for(K)
    row_bytes = 4 * (3 + shf + 1 + 3 + 4 + 6)

    def chunks_of(L):
        g = torch.Generator(device=DEV).manual_seed(L)
        u = lambda *sh: torch.rand(*sh, generator=g, device=DEV)  # noqa: E731
        out = []
        for k in range(K):
            xyz = torch.tensor(cen[k], device=DEV) + (u(L, 3) * 2 - 1) * 3.2
            out.append(H.build_dynamic_hierarchy(xyz, u(L, shf) - 0.5, u(L) * 0.95 + 0.05, u(L, 3) * 0.05 + 0.005,
                                                 u(L, 4) - 0.5))
        return out

    def wall(fn, iters=5, warmup=1):
        ts = []
        for i in range(warmup + iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts[warmup:]))

    out = dict(K=K, sh_floats=shf, row_bytes=row_bytes)
    for rows in sizes:
        print(f"hier_merge: {K} x {rows} rows", file=sys.stderr, flush=True)
        chunks = chunks_of((rows + 1) // 2)
        n_in = sum(int(c[0].shape[0]) for c in chunks)
        whole = wall(lambda: H.merge_dynamic_hierarchies(chunks, cen))
        stages = []
        for _ in range(3):
            ms = {}
            res = H.merge_dynamic_hierarchies(chunks, cen, stage_ms=ms)
            stages.append(ms)
        G = int(res[0].shape[0])
        depth = max(int(c[5][:, 0].max()) for c in chunks) + 1
        st = {k: round(float(np.median([m[k] for m in stages])), 3) for k in H.MERGE_STAGES}
        moved = 2.0 * (G - 1) * row_bytes
        out[str(rows)] = dict(workload=f"{K} chunks x {n_in // K} rows in, {G} rows out, {depth} levels per chunk",
                              kept_fraction=round((G - 1) / n_in, 4), merge_ms=round(whole, 3), rows_in_per_s=round(n_in / (whole * 1e-3)), stage_ms=st,
                              scatter_GBs=round(moved / (st["scatter"] * 1e-3) / 1e9, 1),
                              scatter_hbm_frac=round(moved / (st["scatter"] * 1e-3) / 1e9 / HBM, 3))
        del chunks, res
    chunks = chunks_of(restatement_L)
    host = [tuple(t.cpu().numpy() for t in c) for c in chunks]
    t0 = time.perf_counter()
    ref = MR.merge_ref(host, cen)
    ref_s = time.perf_counter() - t0
    got = H.merge_dynamic_hierarchies(chunks, cen)
    same = bool((got[5].cpu().numpy() == ref["nodes"]).all()) and all(
        bool((g.cpu().numpy().reshape(-1).view(np.int32) == ref[k].reshape(-1).view(np.int32)).all())
        for g, k in zip(got[:5], ("pos", "shs", "alpha", "log_scales", "rot")))
    out["restatement"] = dict(workload=f"recursive numpy restatement, {K} chunks x {restatement_L} leaves, one run",
                              s=round(ref_s, 2), gpu_ms=round(wall(lambda: H.merge_dynamic_hierarchies(chunks, cen)), 3),
                              bitwise_equal=same)
    return out


def bench_spt_nary(rows=250_000, K=4, shf=3, tg=0.02, min_size=64, reps=5):
    """The n-ary SPT path on the merger's output (K chunks of `rows` rows, the chunk recipe of bench_hier_merge) beside
    the binary path on make_dynamic_hierarchy of the same row count: the device build, and the per-view coarse cut of
    the resulting upper tree by the flat cut and by the level walk.  Wall time around a device synchronise, a
    warm-up, then the median of `reps`."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import hier_merge_ref as MR
    from hlgs_core import hierarchy as H
    from hlgs_core import spt
    cen = MR.centers_for(K)

    def wall(fn, warmup=2):
        ts = []
        for _ in range(warmup + reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        ts = ts[warmup:]
        return dict(median_ms=round(float(np.median(ts)), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4),
                    reps=reps)

    g = torch.Generator(device=DEV).manual_seed(rows)
    u = lambda *sh: torch.rand(*sh, generator=g, device=DEV)  # noqa: E731
    L = (rows + 1) // 2
    chunks = [H.build_dynamic_hierarchy(torch.tensor(cen[k], device=DEV) + (u(L, 3) * 2 - 1) * 3.2, u(L, shf) - 0.5,
                                        u(L) * 0.95 + 0.05, u(L, 3) * 0.05 + 0.005, u(L, 4) - 0.5) for k in range(K)]
    pos, _, _, ls, _, nodes, _ = H.merge_dynamic_hierarchies(chunks, cen)
    del chunks
    G = int(nodes.shape[0])
    cc = nodes[:, 2]
    # the volume only the largest 0.5 % of the inner nodes exceed: an upper tree of a few thousand rows over SPTs of a
    # few hundred entries each
    quant = lambda nd, sc, q: float(torch.quantile(torch.exp(sc[nd[:, 2] > 0]).prod(1)[:1_000_000], q))  # noqa: E731
    volume = quant(nodes, ls, 0.995)
    h = S.make_dynamic_hierarchy(S.make_gaussians((G + 1) // 2, 0, S.make_camera(1920, 1080), seed=0), seed=0)
    bn = torch.tensor(h["nodes"])
    bn[:, 3] = torch.where(bn[:, 2] == 2, bn[:, 3], torch.zeros_like(bn[:, 3]))
    bn, bx, bs = bn.to(DEV), torch.tensor(h["means3D"]).to(DEV), torch.log(torch.tensor(h["scales"])).to(DEV)
    bvol = quant(bn, bs, 0.995)

    def leg(nd, p, sc, vol, nary):
        build = lambda: spt.build_hierarchical_spt_device(nd, p, sc, 0, vol, tg, min_size, nary=nary)  # noqa: E731
        t_build = wall(build)
        b = build()
        info = dict(spt.last_device_build)
        un = b["upper_tree_nodes"]
        order = spt.upper_tree_order(un, nary=nary)
        centre = b["upper_tree_xyz"].mean(0).cpu().numpy()
        cam = S.make_camera(1920, 1080, T=-(centre + np.array([0.0, 0.0, -4.0])))
        planes = spt.extract_frustum_planes(cam["projmatrix"])
        args = (un, b["upper_tree_xyz"], b["bounding_sphere_radii"], b["min_distance_squared"], planes, cam["campos"],
                0.05)
        out = dict(rows=int(nd.shape[0]), build=t_build, **info)
        cut = None
        # (the binary level walk goes through the host-count entry point, the flat cut through the device one)
        for name, o in (("cut_flat", order), ("cut_level", None)):
            if name == "cut_flat" and o is None:
                out[name] = "upper tree beyond the flat cut's limits"
                continue
            out[name] = wall(lambda: spt.upper_tree_cut(*args, order=o, nary=nary))
            c = spt.upper_tree_cut(*args, order=o, nary=nary)
            assert cut is None or torch.equal(cut, c)
            cut = c
        out["cut_nodes"] = int(cut.numel())
        return out

    # the volume at the first quartile of the inner-node volumes: no SPT reaches min_SPT_Size, the whole hierarchy is
    # the upper tree (beyond the flat cut's limits) and the level walk runs over all its rows
    whole = dict(nary=leg(nodes, pos, ls, quant(nodes, ls, 0.25), True),
                 binary=leg(bn, bx, bs, quant(bn, bs, 0.25), False))
    assert whole["nary"]["n_spt"] == 0 and whole["nary"]["n_upper"] == G

    # the rank loop of the n-ary level walk: a root with n leaf children is one level whose loop runs n rounds (one block
    # scan and one dependent next_sibling load each); every inner node expands.  Beside it the 299-deep chain of
    # one-child nodes (300 levels of one entry).
    def tree_cut(nd):
        n = nd.shape[0]
        g2 = torch.Generator().manual_seed(n)
        b = spt.build_hierarchical_spt(torch.tensor(nd), torch.randn(n, 3, generator=g2) * 3,
                                       torch.randn(n, 3, generator=g2) * 0.3 - 2, 0, 0.0, tg, 10, nary=True)
        d = [b[k].to(DEV) for k in ("upper_tree_nodes", "upper_tree_xyz", "bounding_sphere_radii",
                                    "min_distance_squared")]
        cam = torch.tensor([0.5, -0.25, 1.0])
        cut = lambda: spt.upper_tree_cut(*d, None, cam, 1e-9, use_frustum=False, nary=True)  # noqa: E731
        return dict(wall(cut), cut_nodes=int(cut().numel()))

    def star(n):
        nd = np.zeros((n + 1, 6), np.int32)
        nd[0] = (0, -1, n, 1, 0, 0)
        for i in range(1, n + 1):
            nd[i] = (1, 0, 0, i + 1, i + 1 if i < n else 0, 0)
        return nd

    chain = np.zeros((300, 6), np.int32)
    for i in range(300):
        chain[i] = (i, i - 1, 1 if i < 299 else 0, i + 1, 0, 0)
    rank_loop = {f"star_{n}_children": tree_cut(star(n)) for n in (2, 300, 3000)}
    rank_loop["chain_299_deep"] = tree_cut(chain)
    per_rank = (rank_loop["star_3000_children"]["median_ms"] - rank_loop["star_300_children"]["median_ms"]) / 2700
    rank_loop["us_per_rank"] = round(per_rank * 1e3, 3)
    return dict(workload=f"merge_dynamic_hierarchies of {K} chunks x {rows} rows -> {G} rows "
                         f"({int((cc == 1).sum())} one-child rows, {int((cc >= 3).sum())} rows with 3+ children, "
                         f"longest list {int(cc.max())}); binary: make_dynamic_hierarchy with {int(bn.shape[0])} rows",
                recipe=dict(target_granularity=tg, min_SPT_Size=min_size, nary_volume=volume, binary_volume=bvol,
                            cut="one 1920x1080 view 4 units from the upper tree's centroid, distance multiplier 0.05"),
                nary=leg(nodes, pos, ls, volume, True), binary=leg(bn, bx, bs, bvol, False),
                whole_hierarchy_as_upper_tree=whole, rank_loop=rank_loop)


def bench_stream(P, views=12):
    from hlgs_core import spt
    from hlgs_core.spt_cache import NAMES, SPTCache
    cam = S.make_camera(1920, 1080)
    h = S.make_dynamic_hierarchy(S.make_gaussians(P, 0, cam, seed=0), seed=0)
    nodes = torch.tensor(h["nodes"])
    nodes[:, 3] = torch.where(nodes[:, 2] == 2, nodes[:, 3], torch.zeros_like(nodes[:, 3]))
    xyz, log_s = torch.tensor(h["means3D"]), torch.log(torch.tensor(h["scales"]))
    G = nodes.shape[0]
    vol, tg, mn = 0.5, 0.00228, 256  # train_post.py:89-91 (granularity and minimum size; volume for this scene scale)
    t0 = time.perf_counter()
    b = spt.build_hierarchical_spt(nodes, xyz, log_s, 0, vol, tg, mn)
    build_s = time.perf_counter() - t0
    widths = dict(xyz=(3,), f_dc=(1, 3), opacity=(1,), scaling=(3,), rotation=(4,), f_rest=(15, 3))
    g = torch.Generator().manual_seed(0)
    storage = {k: torch.randn((G,) + widths[k], generator=g) for k in NAMES}
    t0 = time.perf_counter()
    cache = SPTCache(storage, b, 0, reuse_tolerance=0.05)
    setup_s = time.perf_counter() - t0
    path = [S.make_camera(1920, 1080, T=np.array([0.03 * k, 0.01 * k, 0.2 * math.sin(0.3 * k)])) for k in range(views)]
    step_ms, plan_ms, rows_moved, resident = [], [], [], []
    for k, c in enumerate(path):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ri = cache.step(c["projmatrix"], c["campos"])
        torch.cuda.synchronize()
        step_ms.append((time.perf_counter() - t0) * 1e3)
        pl = cache.last_plan
        rows_moved.append(pl["write_back_indices"].numel() + pl["load_from_disk_indices"].numel())
        resident.append(ri.numel())
        t0 = time.perf_counter()
        cache.plan(c["projmatrix"], c["campos"])
        torch.cuda.synchronize()
        plan_ms.append((time.perf_counter() - t0) * 1e3)
    row_bytes = 4 * 59 * 3  # parameters + two moments per Gaussian
    moved = float(np.median(rows_moved[1:])) * row_bytes
    ms = float(np.median(step_ms[1:]))
    # dense Adam over the resident set (train_post.py:786-812)
    for p in cache.params.values():
        p.grad = torch.randn_like(p)
    R = resident[-1]
    adam_ms = timed(lambda: cache.optimizer_step(100, {k: 1e-3 for k in NAMES}))
    adam_alg = R * 59 * 28
    return dict(workload=f"SPT cache over a {G}-node hierarchy ({P} leaves), {views}-view camera path",
                spt_build_s=round(build_s, 3), n_spt=len(b["SPT_starts"]) - 1, spt_entries=len(b["SPT_max"]),
                upper_tree_nodes=int(b["upper_tree_nodes"].shape[0]), setup_s=round(setup_s, 3),
                resident_median=int(np.median(resident)), view_step_ms=round(ms, 3),
                view_plan_ms=round(float(np.median(plan_ms[1:])), 3), rows_moved_median=int(np.median(rows_moved[1:])),
                host_link_GBs=round(moved / (ms * 1e-3) / 1e9, 2),
                adam=dict(ms=round(adam_ms, 4), alg_GBs=round(adam_alg / (adam_ms * 1e-3) / 1e9, 1),
                          hbm_frac=round(adam_alg / (adam_ms * 1e-3) / 1e9 / HBM, 3), rows=R))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=1_000_000)
    ap.add_argument("--W", type=int, default=1920)
    ap.add_argument("--H", type=int, default=1080)
    ap.add_argument("--only", default="alt,loss,adam,lod")
    ap.add_argument("--knn-sizes", default="250000,1000000,4000000")
    args = ap.parse_args()
    only = set(args.only.split(","))
    out = dict(device=torch.cuda.get_device_name(0), data="synthetic (seeded PCG64)")
    if "alt" in only:
        out["alt"] = bench_alt(args.P, args.W, args.H, 3)
    if "loss" in only:
        out["loss"] = bench_loss(args.W, args.H)
    if "loss_exp" in only:
        out["loss_exp"] = bench_loss_exp(args.W, args.H)
    if "act_reg" in only:
        out["act_reg"] = bench_act_reg(args.P)
    if "adam" in only:
        out["adam"] = bench_adam(args.P)
    if "lod" in only:
        out["lod"], (xyz, _) = bench_lod(args.P, args.W, args.H, 3)
        out["morton"] = bench_morton(xyz)
    if "knn" in only:
        out["knn"] = bench_knn(tuple(int(v) for v in args.knn_sizes.split(",")))
    if "hier_build" in only:
        out["hier_build"] = bench_hier_build()
    if "hier_merge" in only:
        out["hier_merge"] = bench_hier_merge()
    if "spt_nary" in only:
        out["spt_nary"] = bench_spt_nary()
    if "stream" in only:
        out["stream"] = bench_stream(args.P)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
