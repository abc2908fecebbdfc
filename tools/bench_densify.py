#!/usr/bin/env python3
"""One round of the adaptive density control (hlgs_core/densify.py) beside the torch composition it replaces, on one
GPU.

  ours    select (hlgs_density_select), plan (two flag scans and the round's one read-back) and emit (one launch
          over 21 tables: six parameters, twelve Adam moments, three statistics), mode "shrink", two copies, the
          prune mask of min_opacity 0.005 -- what GaussianModel.densify_and_prune computes with its prune restored
  torch   the same round as a caller runs it today: tests/densify_ref.py (the reference lines, torch.cat then a
          boolean mask per table) in float32 on the GPU

Inputs: densify_ref.recipe at --rows rows (default 1M and 4M), SH degree 3 (45 rest floats).  Per size, --settle
untimed rounds of each, then --rounds timed rounds, alternating ours and torch; a round's time is a host clock
around work that ends in a device synchronise (allocation of the output tables included on both sides).  The emit
launch is timed on its own by device events, and the bytes it must move (kept rows read and written, parents read,
new rows written, the row lists) give its achieved rate.  Prints one JSON line; --out also writes it to a file.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "hierarchical-lod-gaussians_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def spread(xs):
    xs = sorted(xs)
    return dict(median=statistics.median(xs), min=xs[0], max=xs[-1], n=len(xs))


def emit_bytes(P, n_kept, n_sel, copies, row_floats, param_floats):
    """Bytes hlgs_densify_emit must move: every kept row read and written in all tables, each parent's parameter row
    read once, every new row written in all tables, and a 4-byte list entry per output row."""
    n_out = n_kept + n_sel * copies
    return 4 * (n_kept * row_floats + n_sel * param_floats + n_out * row_floats + n_out)


def bench(P, rounds, settle):
    import torch

    import densify_ref as R
    from hlgs_core import densify as D
    from hlgs_core import _lib as L

    dev = "cuda"
    inp = R.recipe(P, 45, dev)
    params, m, v = inp["params"], inp["exp_avg"], inp["exp_avg_sq"]
    stats = D.DensityStats(P, dev, _tensors=(inp["grad_accum"], inp["denom"], inp["max_radii2D"]))
    sync = torch.cuda.synchronize

    def ours():
        sel, prune = D.select(stats, params["opacity"], R.GRAD_THRESHOLD, prune_min_opacity=0.005)
        return D.densify_and_prune(params, m, v, stats, sel, prune, seed=0, reset_stats=False)

    def ref():
        sel, prune, _ = R.select_masks(inp["grad_accum"], inp["max_radii2D"], params["opacity"], dtype=torch.float32)
        return R.densify_and_prune(params, m, v, stats.tensors(), sel, prune, "shrink", 2, False, None, False,
                                   torch.float32)

    def timed(f):
        sync()
        t0 = time.perf_counter()
        out = f()
        sync()
        return (time.perf_counter() - t0) * 1e3, out

    for _ in range(settle):
        timed(ours)
        timed(ref)
    t_ours, t_ref = [], []
    for _ in range(rounds):
        a, out = timed(ours)
        b, want = timed(ref)
        t_ours.append(a)
        t_ref.append(b)
    n_kept, n_new = out[4]
    # the same decisions, and the same table up to float32 rounding of the four transformed values per new row
    same_rows = all(out[0][k].shape == want[0][k].shape for k in R.NAMES)
    kept_equal = same_rows and all(torch.equal(out[0][k][:n_kept], want[0][k][:n_kept]) for k in R.NAMES)
    del want

    # the emit launch on its own
    sel, prune = D.select(stats, params["opacity"], R.GRAD_THRESHOLD, prune_min_opacity=0.005)
    scratch, n_kept, n_sel = D._plan(P, sel, prune, False, dev)
    n_out = n_kept + 2 * n_sel
    like = lambda t: torch.empty((n_out,) + tuple(t.shape[1:]), device=dev)  # noqa: E731
    roles = {"xyz": L.DENSIFY_XYZ, "scaling": L.DENSIFY_SCALING, "opacity": L.DENSIFY_OPACITY}
    jobs = [(params[k], like(params[k]), roles.get(k, L.DENSIFY_COPY)) for k in R.NAMES]
    jobs += [(d[k], like(d[k]), L.DENSIFY_ZERO) for d in (m, v) for k in R.NAMES]
    jobs += [(t, like(t), L.DENSIFY_ZERO) for t in stats.tensors()]
    t_emit = []
    for i in range(settle + rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        D._emit(jobs, P, n_kept, n_sel, 2, "shrink", params["rotation"], None, 0, 0, scratch)
        e1.record()
        sync()
        if i >= settle:
            t_emit.append(e0.elapsed_time(e1))
    row_floats = sum(s.numel() // P for s, _, _ in jobs)
    param_floats = sum(params[k].numel() // P for k in R.NAMES)
    nbytes = emit_bytes(P, n_kept, n_sel, 2, row_floats, param_floats)
    emit = spread(t_emit)
    return dict(rows=P, n_kept=n_kept, n_selected=n_sel, n_out=n_out, tables=len(jobs), row_bytes=4 * row_floats,
                round_ms=spread(t_ours), torch_round_ms=spread(t_ref),
                speedup=statistics.median(t_ref) / statistics.median(t_ours), emit_ms=emit, emit_bytes=nbytes,
                emit_tb_per_s=nbytes / (emit["median"] * 1e-3) / 1e12, same_rows=same_rows, kept_rows_equal=kept_equal)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, nargs="+", default=[1_000_000, 4_000_000])
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--settle", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_densify needs a HIP device: there is no CPU path to time")
    line = json.dumps(dict(bench="densify", mode="shrink", copies=2, sh_degree=3,
                           device=torch.cuda.get_device_name(0),
                           sizes=[bench(P, a.rounds, a.settle) for P in a.rows]))
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
