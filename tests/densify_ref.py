"""Torch restatement of the reference's adaptive density control (train_single.py:144-155; scene/gaussian_model.py),
for the tests of hlgs_core/densify.py and tools/bench_densify.py.  Every function takes float32 tensors and a dtype:
torch.float64 is the definition the kernels are compared with (float64 arithmetic from the float32 inputs), and
torch.float32 is the composition a caller of the reference runs today.  Tables are built in the reference's literal
order: the new rows are appended (torch.cat) and the prune mask is applied afterwards."""
import torch

NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
GRAD_THRESHOLD = 0.015  # arguments/__init__.py:177


def recipe(P, sh_rest=45, device="cpu"):
    """The inputs of the tests and of the benchmark for P rows, from seed 300 + P (N = a standard normal sample):
    grad_accum = exp(1.5 N - 7.5) with 2% of the rows (the head of a random permutation) NaN,
    max_radii2D = floor(exp(N + 2)), opacity logits 2.5 N - 1, drawn in this order;
    parameters and moments are normal samples (moments squared for exp_avg_sq), denom small counts."""
    g = torch.Generator().manual_seed(300 + P)
    n = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    grad_accum = torch.exp(1.5 * n(P, 1) - 7.5)
    grad_accum[torch.randperm(P, generator=g)[:int(0.02 * P)]] = float("nan")
    max_radii2D = torch.floor(torch.exp(n(P) + 2))
    opacity = 2.5 * n(P, 1) - 1
    denom = torch.randint(0, 50, (P, 1), generator=g).float()
    params = dict(xyz=n(P, 3) * 3, f_dc=n(P, 1, 3), f_rest=n(P, sh_rest // 3, 3) * 0.1, opacity=opacity,
                  scaling=n(P, 3) * 0.5 - 2, rotation=n(P, 4))
    params["rotation"][params["rotation"].norm(dim=1) < 1e-3] = 1.0
    exp_avg = {k: n(*v.shape) * 1e-3 for k, v in params.items()}
    exp_avg_sq = {k: n(*v.shape) ** 2 * 1e-6 for k, v in params.items()}
    to = lambda d: {k: v.to(device).contiguous() for k, v in d.items()}  # noqa: E731
    return dict(params=to(params), exp_avg=to(exp_avg), exp_avg_sq=to(exp_avg_sq), grad_accum=grad_accum.to(device),
                denom=denom.to(device), max_radii2D=max_radii2D.to(device))


def stats_update(dL_dmean2D, radii, grad_accum, denom, max_radii2D, dtype=torch.float64):
    """train_single.py:147-148 and gaussian_model.py:1527-1530 for the rows with radii > 0 (the visibility filter of
    gaussian_renderer): max_radii2D = max(max_radii2D, radii), grad_accum = max(|grad[:, :2]|, grad_accum),
    denom += 1.  Returns new float32 tensors."""
    vis = radii > 0
    mr, ga, dn = max_radii2D.clone(), grad_accum.clone(), denom.clone()
    mr[vis] = torch.max(max_radii2D[vis], radii[vis].to(torch.float32))                      # train_single.py:147
    norm = torch.norm(dL_dmean2D[:, :2].to(dtype), dim=-1, keepdim=True)                      # :1527
    ga[vis] = torch.max(norm[vis], grad_accum[vis].to(dtype)).to(torch.float32)
    dn[vis] += 1                                                                              # :1530
    return ga, dn, mr


def select_terms(grad_accum, max_radii2D, opacity_raw, dtype=torch.float64):
    """(score, opacity) of the selection rule: grads with NaN as 0 (:1508) times max_radii2D times opacity^(1/5)
    (:1458), and the activated opacity (:1460, :1512)."""
    g = grad_accum.reshape(-1).to(dtype).clone()
    g[g.isnan()] = 0.0
    o = torch.sigmoid(opacity_raw.reshape(-1).to(dtype))
    return g * max_radii2D.to(dtype) * torch.pow(o, 1 / 5.0), o


def select_masks(grad_accum, max_radii2D, opacity_raw, grad_threshold=GRAD_THRESHOLD, protect_rows=0, leaf=None,
                 densify_min_opacity=0.15, prune_min_opacity=0.005, dtype=torch.float64):
    """(select, prune, near): the masks of :1458-1468 and :1512-1514, and the rows whose score or opacity lies within
    a relative 1e-5 of one of the three thresholds (a rounding could decide them either way)."""
    score, o = select_terms(grad_accum, max_radii2D, opacity_raw, dtype)
    sel = torch.logical_and(score >= grad_threshold, o > densify_min_opacity)
    if leaf is not None:
        sel = torch.logical_and(sel, leaf.bool())                                             # :1468
    sel[:protect_rows] = False                                                                # :1465-1466
    if prune_min_opacity < 0:
        prune = torch.zeros_like(sel)
    else:
        prune = o < prune_min_opacity                                                         # :1512
        prune[:protect_rows] = False                                                          # :1513-1514
    rel = lambda v, t: (v - t).abs() <= 1e-5 * abs(t)  # noqa: E731
    near = rel(score, grad_threshold) | rel(o, densify_min_opacity)
    if prune_min_opacity >= 0:
        near |= rel(o, prune_min_opacity)
    return sel, prune, near


def rotation_matrix(q):
    """build_rotation (utils/general_utils.py): the quaternion is normalised, then R(r, x, y, z)."""
    q = q / q.norm(dim=1, keepdim=True)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                     2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                     2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], dim=1)
    return R.reshape(-1, 3, 3)


def new_rows(params, sel, mode, copies=2, noise=None, dtype=torch.float64):
    """The six extension tensors of densify_and_clone (:1420-1426), densify (:1473-1479, "shrink") or
    densify_and_split (:1367-1376) for the selected rows; transformed values in dtype, copied ones untouched."""
    N = copies
    rep = lambda t: t[sel].repeat_interleave(repeats=N, dim=0)  # noqa: E731
    new = {k: rep(params[k]) for k in NAMES}
    if mode == "shrink":
        new["scaling"] = torch.log(rep(torch.exp(params["scaling"].to(dtype))) / (0.8 * N))   # :1474
        y = rep(torch.sigmoid(params["opacity"].to(dtype))) / (0.8 * N)                       # :1478
        new["opacity"] = torch.log(y / (1 - y))
    elif mode == "split":
        stds = rep(torch.exp(params["scaling"].to(dtype)))                                    # :1367
        samples = stds * noise.to(dtype)                                                      # :1369, normal(0, stds)
        rots = rep(rotation_matrix(params["rotation"].to(dtype)))                             # :1370
        new["xyz"] = torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + rep(params["xyz"].to(dtype))  # :1371
        new["scaling"] = torch.log(stds / (0.7 * N))                                          # :1372
    else:
        assert mode == "clone"  # :1421 writes log(exp(s)); the project copies s (include/hlgs.h)
    return new


def densify_and_prune(params, exp_avg, exp_avg_sq, stats, sel, prune=None, mode="shrink", copies=2,
                      drop_selected=False, noise=None, reset_stats=True, dtype=torch.float64):
    """The round in the reference's order: cat_tensors_to_optimizer (:1302-1306: the new rows behind the old ones,
    their moments zero), then the mask of prune_points (:1254-1258, :1279-1282) over the grown tables, with the new
    rows never pruned (:1401).  stats = (grad_accum, denom, max_radii2D).  Returns (params, exp_avg, exp_avg_sq, stats)
    with the transformed tables in dtype."""
    sel = sel.bool()
    new = new_rows(params, sel, mode, copies, noise, dtype)
    n_new = int(new["xyz"].shape[0])
    gone = torch.zeros_like(sel) if prune is None else prune.bool().clone()
    if drop_selected:
        gone |= sel                                                                           # :1401
    valid = ~torch.cat([gone, torch.zeros(n_new, dtype=torch.bool, device=sel.device)])       # :1268
    out_p, out_m, out_v = {}, {}, {}
    for k in NAMES:
        wide = new[k].dtype
        out_p[k] = torch.cat([params[k].to(wide), new[k]], dim=0)[valid]                      # :1306, :1258
        out_m[k] = torch.cat([exp_avg[k], torch.zeros_like(new[k], dtype=torch.float32)], dim=0)[valid]      # :1302
        out_v[k] = torch.cat([exp_avg_sq[k], torch.zeros_like(new[k], dtype=torch.float32)], dim=0)[valid]   # :1303
    n_out = int(valid.sum())
    if reset_stats:                                                                           # :1343-1345
        out_s = tuple(torch.zeros((n_out,) + tuple(t.shape[1:]), device=t.device) for t in stats)
    else:                                                                                     # :1279-1282
        out_s = tuple(torch.cat([t, torch.zeros((n_new,) + tuple(t.shape[1:]), device=t.device)], dim=0)[valid]
                      for t in stats)
    return out_p, out_m, out_v, out_s


def reset_opacity(opacity_raw, protect_rows=0, max_opacity=0.01):
    """reset_opacity (:1214-1218) without its inverse_sigmoid(sigmoid(x)) round trip: rows >= protect_rows whose
    float64 sigmoid exceeds max_opacity take float32(logit(max_opacity)); the others are unchanged."""
    import math
    out = opacity_raw.clone()
    over = torch.sigmoid(opacity_raw.double()) > max_opacity
    over[:protect_rows] = False
    out[over] = torch.tensor(math.log(max_opacity / (1 - max_opacity)), dtype=torch.float64).float()
    return out
