"""The adaptive density control of chunk training (train_single.py:144-155) on the HIP path: what happens between two
optimizer steps to change the number of Gaussians.

  DensityStats.update_(...)   add_densification_stats (train_single.py:147-148, scene/gaussian_model.py:1527-1530)
  select(...)                 the masks of densify / densify_and_prune (:1458-1468, :1508, :1512-1514)
  densify_and_prune(...)      densify (:1473-1479), densify_and_clone (:1420-1426) or densify_and_split (:1367-1376)
                              with prune_points (:1249-1282) and cat_tensors_to_optimizer (:1294-1314): every parameter,
                              both Adam moments and the statistics move in one launch (hlgs_densify_emit)
  reset_opacity_(...)         reset_opacity (:1214-1218, :1237-1238)
  rebind_optimizer(...)       the optimizer side of cat_tensors_to_optimizer / _prune_optimizer /
                              replace_tensor_to_optimizer (:1232-1314), by group name; host code, any device

params, exp_avg, exp_avg_sq: dicts over NAMES (the group names of training_setup) -> contiguous float32 device tensors
of P rows.  The reference's own methods cannot be called as written (include/hlgs.h says why); their arithmetic is the
contract.  A round is a function of its inputs, the seed and the round number (csrc/hlgs_rng.h).  There is no CPU
fallback: without the library or a HIP device the compute functions raise, after their shape errors.
"""
import torch

from hlgs_core import _lib as L

NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
_ROLES = {"xyz": L.DENSIFY_XYZ, "scaling": L.DENSIFY_SCALING, "opacity": L.DENSIFY_OPACITY}


def _rows(t, P, what, dtype=torch.float32, width=None):
    if t.dtype != dtype or not t.is_contiguous() or t.dim() < 1 or int(t.shape[0]) != P:
        raise RuntimeError(f"{what} must be a contiguous {str(dtype).replace('torch.', '')} tensor of {P} rows")
    if width is not None and t.numel() != P * width:
        raise RuntimeError(f"{what} must have {width} element(s) per row")
    return t


class DensityStats:
    """xyz_gradient_accum (P, 1), denom (P, 1) and max_radii2D (P) of GaussianModel (:1343-1345)."""

    def __init__(self, P, device="cuda", *, _tensors=None):
        self.P = int(P)
        if _tensors is None:
            _tensors = (torch.zeros((self.P, 1), device=device), torch.zeros((self.P, 1), device=device),
                        torch.zeros((self.P,), device=device))
        self.grad_accum, self.denom, self.max_radii2D = _tensors

    def tensors(self):
        return self.grad_accum, self.denom, self.max_radii2D

    def update_(self, means2D_grad, radii):
        """For the rows with radii > 0: max_radii2D = max(max_radii2D, radii), grad_accum = max(grad_accum,
        |means2D_grad[:, :2]|), denom += 1 (train_single.py:147-148, :1527-1530), in place, one pass."""
        P = self.P
        _rows(means2D_grad, P, "means2D_grad", width=3)
        _rows(radii, P, "radii", torch.int32, 1)
        lib = L.load()
        L.require_gpu(means2D_grad, radii, *self.tensors())
        L.check(lib.hlgs_density_stats(P, L.ptr(means2D_grad), L.ptr(radii), L.ptr(self.grad_accum),
                                       L.ptr(self.denom), L.ptr(self.max_radii2D), L.stream()))
        return self


def select(stats, opacity_raw, grad_threshold, *, protect_rows=0, leaf=None, densify_min_opacity=0.15,
           prune_min_opacity=-1.0):
    """(select, prune) uint8 masks of P rows.  With o = sigmoid(opacity_raw) and g = grad_accum (NaN as 0, :1508):
    select = g max_radii2D o^(1/5) >= grad_threshold and o > densify_min_opacity and leaf and row >= protect_rows
    (:1458-1468); prune = o < prune_min_opacity and row >= protect_rows (:1512-1514), all zero when
    prune_min_opacity < 0.  The reference's values: grad_threshold 0.015, 0.15, 0.005."""
    P = stats.P
    _rows(opacity_raw, P, "opacity_raw", width=1)
    if leaf is not None:
        if leaf.dtype == torch.bool:
            leaf = leaf.view(torch.uint8)
        _rows(leaf, P, "leaf", torch.uint8, 1)
    lib = L.load()
    L.require_gpu(opacity_raw, leaf, *stats.tensors())
    dev = opacity_raw.device
    sel = torch.empty((P,), dtype=torch.uint8, device=dev)
    prune = torch.empty((P,), dtype=torch.uint8, device=dev)
    L.check(lib.hlgs_density_select(P, L.ptr(stats.grad_accum), L.ptr(stats.max_radii2D), L.ptr(opacity_raw),
                                    L.ptr(leaf), float(grad_threshold), float(densify_min_opacity),
                                    float(prune_min_opacity), int(protect_rows), L.ptr(sel), L.ptr(prune), L.stream()))
    return sel, prune


_pinned = {}


def _counts_host():
    """Two pinned int32 words for the plan's read-back, one buffer per process (the plan synchronises before it
    returns, so the buffer is free again)."""
    if "c" not in _pinned:
        _pinned["c"] = torch.zeros((2,), dtype=torch.int32).pin_memory()
    return _pinned["c"]


def _mask(m, P, what):
    if m.dtype == torch.bool:
        m = m.view(torch.uint8)
    return _rows(m, P, what, torch.uint8, 1)


def densify_and_prune(params, exp_avg, exp_avg_sq, stats, select, prune=None, *, mode="shrink", copies=2,
                      drop_selected=False, seed, round=0, noise=None, reset_stats=True):
    """One round.  Returns (params, exp_avg, exp_avg_sq, stats, (n_kept, n_new)), all new tensors of
    n_kept + n_new rows: first the kept rows (not pruned, and not selected when drop_selected) in ascending order, bit
    for bit in every table, then `copies` new rows per selected row in ascending parent order (:1473, :1306).  New
    rows: mode "clone" copies the parent; "shrink" (densify, what GaussianModel.densify_and_prune calls) divides the
    activated scale and opacity by 0.8 copies; "split" draws xyz from the parent's Gaussian and divides the activated
    scale by 0.7 copies.  Their moments are zero.  xi of "split": noise (n_new, 3) when given, else the normals of
    (seed, stream = round).  reset_stats: the statistics come back zeroed (:1343-1345, :1518); otherwise the kept
    rows' statistics are compacted (:1279-1282) and the new rows' are 0.  The defaults are the reference as written
    (shrink, two copies, parents kept, nothing pruned); mode="split", drop_selected=True with a prune mask is
    upstream's densify_and_split + prune."""
    if set(params) != set(NAMES) or set(exp_avg) != set(NAMES) or set(exp_avg_sq) != set(NAMES):
        raise RuntimeError(f"params, exp_avg and exp_avg_sq are dicts over {NAMES}")
    if mode not in L.DENSIFY_MODES:
        raise RuntimeError(f"mode must be one of {sorted(L.DENSIFY_MODES)}")
    copies = int(copies)
    if copies < 1:
        raise RuntimeError("copies must be at least 1")
    P = int(params["xyz"].shape[0])
    if stats.P != P:
        raise RuntimeError(f"stats hold {stats.P} rows, the parameters {P}")
    for k, w in zip(NAMES, (3, 3, None, 1, 3, 4)):
        _rows(params[k], P, k, width=w)
        for d, what in ((exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
            if _rows(d[k], P, f"{what}[{k}]").shape != params[k].shape:
                raise RuntimeError(f"{what}[{k}] must have the shape of {k}")
    select = _mask(select, P, "select")
    if prune is not None:
        prune = _mask(prune, P, "prune")
    L.load()
    tensors = [d[k] for d in (params, exp_avg, exp_avg_sq) for k in NAMES]
    L.require_gpu(select, prune, noise, *tensors, *stats.tensors())
    dev = params["xyz"].device
    scratch, n_kept, n_sel = _plan(P, select, prune, drop_selected, dev)
    n_new = n_sel * copies
    n_out = n_kept + n_new
    if noise is not None:
        _rows(noise, n_new, "noise", width=3)
    elif mode == "split" and seed is None:
        raise RuntimeError("split needs a seed or the noise itself")

    def like(t):
        return torch.empty((n_out,) + tuple(t.shape[1:]), dtype=t.dtype, device=dev)

    out = [{k: like(d[k]) for k in NAMES} for d in (params, exp_avg, exp_avg_sq)]
    jobs = [(params[k], out[0][k], _ROLES.get(k, L.DENSIFY_COPY)) for k in NAMES]
    jobs += [(d[k], o[k], L.DENSIFY_ZERO) for d, o in ((exp_avg, out[1]), (exp_avg_sq, out[2])) for k in NAMES]
    if reset_stats:
        new_stats = DensityStats(n_out, dev)
    else:
        new_stats = DensityStats(n_out, dev, _tensors=tuple(like(t) for t in stats.tensors()))
        jobs += [(s, d, L.DENSIFY_ZERO) for s, d in zip(stats.tensors(), new_stats.tensors())]
    _emit(jobs, P, n_kept, n_sel, copies, mode, params["rotation"], noise, seed, round, scratch)
    return out[0], out[1], out[2], new_stats, (n_kept, n_new)


def _aligned(scratch):
    p = scratch.data_ptr()
    return L._vp(p + -p % 256)


def _plan(P, select, prune, drop_selected, dev):
    """hlgs_densify_plan: (scratch holding the row lists, n_kept, n_selected); the round's one host synchronisation."""
    lib = L.load()
    scratch = torch.empty((lib.hlgs_densify_scratch_size(P) + 256,), dtype=torch.uint8, device=dev)
    counts = _counts_host()
    L.check(lib.hlgs_densify_plan(P, L.ptr(select), L.ptr(prune), int(bool(drop_selected)), _aligned(scratch),
                                  L._vp(counts.data_ptr()), L.stream()))
    return scratch, int(counts[0]), int(counts[1])


def _emit(jobs, P, n_kept, n_sel, copies, mode, rotation, noise, seed, round, scratch):
    """hlgs_densify_emit over jobs = [(source table, destination table, role)]: one launch."""
    tabs = (L.DensifyTable * len(jobs))()
    for i, (src, dst, role) in enumerate(jobs):
        row_bytes = 4 * (src.numel() // P) if P else 0
        tabs[i] = L.DensifyTable(src.data_ptr() if src.numel() else None, dst.data_ptr() if dst.numel() else None,
                                 row_bytes, role)
    if n_kept + n_sel * copies:
        L.check(L.load().hlgs_densify_emit(len(jobs), tabs, P, n_kept, n_sel, copies, L.DENSIFY_MODES[mode],
                                           L.ptr(rotation), L.ptr(noise), int(seed or 0), int(round),
                                           _aligned(scratch), L.stream()))


def reset_opacity_(opacity_raw, exp_avg, exp_avg_sq, *, protect_rows=0, max_opacity=0.01):
    """reset_opacity (:1214-1218) in place, one pass: rows >= protect_rows whose sigmoid exceeds max_opacity take
    logit(max_opacity); every other row keeps its bits.  Both moments of the opacity tensor are zeroed (:1237-1238)."""
    P = int(opacity_raw.shape[0])
    _rows(opacity_raw, P, "opacity_raw", width=1)
    _rows(exp_avg, P, "exp_avg", width=1)
    _rows(exp_avg_sq, P, "exp_avg_sq", width=1)
    if not 0.0 < float(max_opacity) < 1.0:
        raise RuntimeError("max_opacity must lie in (0, 1)")
    lib = L.load()
    L.require_gpu(opacity_raw, exp_avg, exp_avg_sq)
    L.check(lib.hlgs_opacity_reset(P, int(protect_rows), float(max_opacity), L.ptr(opacity_raw), L.ptr(exp_avg),
                                   L.ptr(exp_avg_sq), L.stream()))
    return opacity_raw


def rebind_optimizer(optimizer, params, exp_avg=None, exp_avg_sq=None):
    """Put params[name] into the optimizer's group of that name as a new nn.Parameter and move the group's state to
    it with exp_avg[name] / exp_avg_sq[name] as its moments: the group-by-name replacement of
    cat_tensors_to_optimizer, _prune_optimizer and replace_tensor_to_optimizer (:1232-1314).  Groups without state
    (no step taken yet) get none, as in the reference; other state entries (step) are kept.  Works on any torch
    optimizer whose state uses exp_avg / exp_avg_sq, on any device.  Returns {name: nn.Parameter}."""
    new = {}
    for group in optimizer.param_groups:
        name = group.get("name")
        if name not in params:
            continue
        if len(group["params"]) != 1:
            raise RuntimeError(f"group {name!r} must hold exactly one parameter")
        old = group["params"][0]
        state = optimizer.state.pop(old, None)
        p = torch.nn.Parameter(params[name].detach().requires_grad_(True))
        if state is not None and exp_avg is not None and exp_avg_sq is not None:
            for key, d in (("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq)):
                if d[name].shape != p.shape:
                    raise RuntimeError(f"{key}[{name}] must have the shape of the parameter")
                state[key] = d[name]
            optimizer.state[p] = state
        group["params"][0] = p
        new[name] = p
    missing = set(params) - set(new)
    if missing:
        raise RuntimeError(f"the optimizer has no group named {sorted(missing)}")
    return new
