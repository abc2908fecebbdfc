"""Timings of the MCMC densification pieces on one GPU; not part of bench.py.

  python tools/mcmc_bench.py noise   [--rows 600000]
  python tools/mcmc_bench.py sample  [--n 16000000 --num 1600000 --host-n 50000000]
  python tools/mcmc_bench.py round   [--leaves 1000000] [--spt-device]
  python tools/mcmc_bench.py spt     [--leaves 1000000]   host and device SPT build on one hierarchy, one process
  python tools/mcmc_bench.py select  [--leaves 1000000 --merged-rows 250000 --out FILE]   the relocation's selection:
                                     host (binary) against device (child lists), and the device on a merged K = 4 scene

Every figure is the median (min-max) of --reps calls after --warmup calls, timed with device events around a call
that ends in a synchronise where the call itself does not.  One JSON line per measurement."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "hierarchical-lod-gaussians_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return dict(median_ms=round(ms[len(ms) // 2], 4), min_ms=round(ms[0], 4), max_ms=round(ms[-1], 4), reps=reps)


def report(name, **kw):
    print(json.dumps(dict(measurement=name, **kw)), flush=True)


def bench_noise(a):
    import mcmc_ref as R
    from hlgs_core import mcmc
    P = a.rows
    g = torch.Generator().manual_seed(0)
    op = (torch.randn(P, 1, generator=g) * 2).cuda()
    sc = (torch.randn(P, 3, generator=g) * 0.5 - 2).cuda()
    rot = torch.randn(P, 4, generator=g).cuda()
    means = torch.zeros(P, 3, device="cuda")

    def torch_step():
        means.add_(R.noise_delta(op, sc, rot, torch.randn_like(means), 5e5, 1.6e-4, torch.float32))
    report("noise_kernel", rows=P, bytes_per_row=56,
           **timed(lambda: mcmc.position_noise_(means, op, sc, rot, 5e5, 1.6e-4, seed=1, step=3), a.warmup, a.reps))
    report("noise_torch_composition", rows=P, **timed(torch_step, a.warmup, a.reps))


def bench_sample(a):
    from hlgs_core import mcmc
    n, num = a.n, a.num
    g = torch.Generator().manual_seed(0)
    logits = torch.randn(n, 1, generator=g)
    dev = logits.cuda()
    report("sample_device", n=n, num=num, **timed(lambda: mcmc.sample_alive(dev, num, seed=1), a.warmup, a.reps))
    nt = min(n, 2 ** 24)
    probs = torch.sigmoid(dev[:nt, 0])
    report("torch_multinomial", n=nt, num=num,
           **timed(lambda: torch.bincount(torch.multinomial(probs, num, replacement=True), minlength=nt), a.warmup,
                   a.reps))
    del dev, probs, logits
    # packed pinned rows (SPTCache.host: 192 floats per Gaussian, the opacity at word 6)
    G = a.host_n
    host = torch.zeros((G, 192), dtype=torch.float32, pin_memory=True)
    host[:, 6] = torch.randn(G, generator=g)
    op = host[:, 6:7]
    report("sample_packed_host_rows_in_place", n=G, num=num, line_bytes_per_candidate=64,
           **timed(lambda: mcmc.sample_alive(op, num, seed=1), 1, max(3, a.reps // 4)))

    def copy_first():
        mcmc.sample_alive(op.cuda(), num, seed=1)
    report("sample_after_torch_copy_of_the_column", n=G, num=num, **timed(copy_first, 1, max(3, a.reps // 4)))
    col = op.cuda()
    report("sample_device_column_only", n=G, num=num,
           **timed(lambda: mcmc.sample_alive(col, num, seed=1), 1, max(3, a.reps // 4)))


def bench_spt(a):
    """The host build and the device build of the SPTs on the same hierarchy (the round's recipe).  The host build
    takes pageable host tensors, as densify_round hands them over; the device build takes the nodes on the host and
    the parameter columns as strided views of a packed pinned table (SPTCache.storage), and is also timed on
    device-resident contiguous columns.  staging: its packing and validation kernels alone (HLGS_SPT_STAGE_PACK)."""
    from hlgs_core import spt
    from hlgs_core import synthetic as S
    sky = 4
    h = S.make_dynamic_hierarchy(S.make_gaussians(a.leaves, 0, S.make_camera(256, 192), seed=8), skybox_points=sky,
                                 seed=8)
    nodes = torch.tensor(h["nodes"])
    G = int(nodes.shape[0])
    xyz, scaling = torch.tensor(h["means3D"]), torch.log(torch.tensor(h["scales"]))
    host = torch.zeros((G, 192), dtype=torch.float32, pin_memory=True)  # SPTCache.host: xyz at word 0, scaling at 7
    host[:, 0:3] = xyz
    host[:, 7:10] = scaling
    vx, vs = host[:, 0:3], host[:, 7:10]
    args = (sky, a.volume, a.granularity, 256)
    want = spt.build_hierarchical_spt(nodes, xyz, scaling, *args)
    got = spt.build_hierarchical_spt_device(nodes, vx, vs, *args)
    info = dict(spt.last_device_build)
    for k in ("SPT_starts", "SPT_gaussian_indices", "SPT_root_hierarchy_indices", "upper_tree_nodes"):
        assert torch.equal(got[k].cpu(), want[k]), k
    reps = max(3, a.reps // 2)
    t_host = timed(lambda: spt.build_hierarchical_spt(nodes, xyz, scaling, *args), 1, reps)
    t_dev = timed(lambda: spt.build_hierarchical_spt_device(nodes, vx, vs, *args), a.warmup, reps)
    nd, dx, ds = nodes.cuda(), xyz.cuda(), scaling.cuda()
    t_res = timed(lambda: spt.build_hierarchical_spt_device(nd, dx, ds, *args), a.warmup, reps)
    t_pack = timed(lambda: spt.build_hierarchical_spt_device(nd, vx, vs, *args, stages=1), a.warmup, reps)
    t_pack_res = timed(lambda: spt.build_hierarchical_spt_device(nd, dx, ds, *args, stages=1), a.warmup, reps)
    report("spt_build", rows=G, **info, host=t_host, device_pinned_views=t_dev, device_resident=t_res,
           staging_pinned_views=t_pack, staging_resident=t_pack_res,
           device_over_host_min=round(t_dev["min_ms"] / t_host["min_ms"], 4))


def bench_round(a):
    from hlgs_core import mcmc, spt
    from hlgs_core import synthetic as S
    from hlgs_core.spt_cache import NAMES, SPTCache
    sky = 4
    h = S.make_dynamic_hierarchy(S.make_gaussians(a.leaves, 0, S.make_camera(256, 192), seed=8), skybox_points=sky,
                                 seed=8)
    size = h["nodes"].shape[0]
    cap = int(1.1 * size)
    nodes = torch.zeros((cap, 6), dtype=torch.int32)
    nodes[:size] = torch.tensor(h["nodes"])
    shapes = dict(xyz=(3,), f_dc=(1, 3), opacity=(1,), scaling=(3,), rotation=(4,), f_rest=(15, 3))
    storage = {k: torch.zeros((cap,) + shapes[k]) for k in NAMES}
    storage["xyz"][:size] = torch.tensor(h["means3D"])
    storage["scaling"][:size] = torch.log(torch.tensor(h["scales"]))
    storage["rotation"][:size] = torch.tensor(h["rotations"])
    op = torch.tensor(h["opacities"]).clamp(0.01, 0.99)
    storage["opacity"][:size] = torch.log(op / (1 - op))
    rng = np.random.default_rng(8)
    leaves = torch.where(nodes[:size, 2] == 0)[0]
    low = leaves[torch.tensor(rng.choice(len(leaves), size=len(leaves) // 20, replace=False))]
    storage["opacity"][low] = float(np.log(0.001 / 0.999))
    args = dict(SPT_Root_Volume=a.volume, target_granularity=a.granularity, min_SPT_Size=256)
    b = spt.build_hierarchical_spt(nodes[:size], storage["xyz"][:size], storage["scaling"][:size], sky, *args.values())
    cache = SPTCache(storage, b, sky)
    cam = S.make_camera(320, 240, T=np.array([0.0, 0.0, 0.3]))
    cache.step(cam["projmatrix"], cam["campos"])
    resident = int(cache.render_indices.numel())

    def clock():
        torch.cuda.synchronize()
        return time.perf_counter()
    t = [clock()]
    cache.reset()
    t.append(clock())
    dead = torch.where(cache.storage["opacity"][:size, 0] <= float(np.log(0.005 / 0.995)))[0]
    new_size = mcmc.add_new_gs(cache.storage, nodes, size, 10 ** 9, seed=1)
    t.append(clock())
    mask = torch.zeros(new_size, dtype=torch.bool)
    mask[dead] = True
    mask &= nodes[:new_size, 2] == 0
    moved = mcmc.relocate_gs(cache.storage, cache.opt_storage, nodes, mask, new_size, sky, seed=1)
    t.append(clock())
    build = spt.build_hierarchical_spt_device if a.spt_device else spt.build_hierarchical_spt
    b = build(nodes[:new_size], cache.storage["xyz"][:new_size], cache.storage["scaling"][:new_size], sky,
              *args.values())
    t.append(clock())
    cache.reset(b)
    t.append(clock())
    names = ("reset", "spawn", "relocate", "spt_rebuild", "reset_with_spt")
    report("densify_round", spt_on_device=bool(a.spt_device), size=size, new_size=new_size, resident_rows=resident, relocated=moved, runs=1,
           **{f"{k}_ms": round(1e3 * (y - x), 2) for k, x, y in zip(names, t, t[1:])})


def bench_select(a):
    """The selection of the relocation: the device selection over child lists (select_relocation_nary: the upload of
    the node table and the flags, the count, its read-back, the emit, and the read-back of the group lists; the alive
    list stays on the device, where the sampler reads it) beside the host selection of the binary round
    (select_relocation: nonzero and isin over every row) on the binary scene of `round` with 5 % dead leaves, and the
    device selection on the merged K = 4 scene of tools/bench_extras.py's spt_nary.  Wall time around a synchronise."""
    import hier_merge_ref as MR
    from hlgs_core import hierarchy as H
    from hlgs_core import mcmc
    from hlgs_core import synthetic as S

    def wall(fn):
        ts = []
        for _ in range(a.warmup + a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        ts = sorted(ts[a.warmup:])
        return dict(median_ms=round(ts[len(ts) // 2], 4), min_ms=round(ts[0], 4), max_ms=round(ts[-1], 4), reps=a.reps)

    def flags(nodes, sky):
        rng = np.random.default_rng(8)
        leaves = torch.where(nodes[sky:, 2] == 0)[0] + sky
        mask = torch.zeros(nodes.shape[0], dtype=torch.bool)
        mask[leaves[torch.tensor(rng.choice(len(leaves), size=len(leaves) // 20, replace=False))]] = True
        return mask

    def device_select(nodes, mask, sky):
        out = mcmc.select_relocation_nary(nodes, mask, nodes.shape[0], sky)
        return tuple(t.cpu() for t in out[:4]) + (out[4],)

    results = {}
    sky = 4
    print(f"select: building the binary scene of {a.leaves} leaves", file=sys.stderr, flush=True)
    h = S.make_dynamic_hierarchy(S.make_gaussians(a.leaves, 0, S.make_camera(256, 192), seed=8), skybox_points=sky,
                                 seed=8)
    nodes = torch.tensor(h["nodes"])
    mask = flags(nodes, sky)
    size = int(nodes.shape[0])
    dead, sib, alive = mcmc.select_relocation(nodes, mask, size)
    gp, gs, st, fr, al = device_select(nodes, mask, sky)
    assert torch.equal(fr.long(), torch.stack([dead, sib.long()], 1).reshape(-1)) and torch.equal(gs, sib)
    assert torch.equal(al.cpu().long(), alive) and torch.equal(gp, nodes[dead, 1])
    results["binary"] = dict(rows=size, dead_flags=int(mask.sum()), groups=int(gp.numel()), alive=int(al.numel()),
                             host_select_relocation=wall(lambda: mcmc.select_relocation(nodes, mask, size)),
                             device_select_relocation_nary=wall(lambda: device_select(nodes, mask, sky)))
    b = results["binary"]
    b["device_over_host_median"] = round(b["device_select_relocation_nary"]["median_ms"] /
                                         b["host_select_relocation"]["median_ms"], 4)
    report("select_binary", **b)
    # the merged scene of bench_extras.bench_spt_nary: K = 4 chunks of 250,000 rows
    K, rows, shf = 4, a.merged_rows, 3
    cen = MR.centers_for(K)
    g = torch.Generator(device="cuda").manual_seed(rows)
    u = lambda *sh: torch.rand(*sh, generator=g, device="cuda")  # noqa: E731
    L = (rows + 1) // 2
    chunks = [H.build_dynamic_hierarchy(torch.tensor(cen[k], device="cuda") + (u(L, 3) * 2 - 1) * 3.2, u(L, shf) - 0.5,
                                        u(L) * 0.95 + 0.05, u(L, 3) * 0.05 + 0.005, u(L, 4) - 0.5) for k in range(K)]
    nodes = H.merge_dynamic_hierarchies(chunks, cen)[5].cpu()
    del chunks
    mask = flags(nodes, 0)
    gp, gs, st, fr, al = device_select(nodes, mask, 0)
    results["merged_k4"] = dict(rows=int(nodes.shape[0]), longest_list=int(nodes[:, 2].max()),
                                dead_flags=int(mask.sum()), groups=int(gp.numel()),
                                promote_groups=int((gs >= 0).sum()), freed_rows=int(fr.numel()),
                                alive=int(al.numel()),
                                device_select_relocation_nary=wall(lambda: device_select(nodes, mask, 0)))
    report("select_merged_k4", **results["merged_k4"])
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(measurement="mcmc_select", warmup=a.warmup, **results), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["noise", "sample", "round", "spt", "select"])
    ap.add_argument("--merged-rows", type=int, default=250_000)  # select: rows per chunk of the merged K = 4 scene
    ap.add_argument("--out", default=None)  # select: also write the results to this JSON file
    ap.add_argument("--rows", type=int, default=600_000)
    ap.add_argument("--n", type=int, default=16_000_000)
    ap.add_argument("--num", type=int, default=1_600_000)
    ap.add_argument("--host-n", type=int, default=50_000_000)
    ap.add_argument("--leaves", type=int, default=1_000_000)
    ap.add_argument("--volume", type=float, default=0.5)  # config #5 (bench.py): 0.5, 0.00228, 256
    ap.add_argument("--granularity", type=float, default=0.00228)
    ap.add_argument("--spt-device", action="store_true")  # round: rebuild the SPTs with the device build
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mcmc_bench.py measures on the GPU; none is present")
    {"noise": bench_noise, "sample": bench_sample, "round": bench_round, "spt": bench_spt,
     "select": bench_select}[a.what](a)
