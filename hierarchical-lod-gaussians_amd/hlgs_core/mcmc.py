"""The MCMC densification round of train_post.py (MCMC_Densification, on by default there: :70-75, 707-789) and its
position noise (:868-878) on the HIP path.

  sample_alive(...)        GaussianModel._sample_alives (scene/gaussian_model.py:1580-1586) with the sigmoid
                           probabilities of its callers (:1614, :1714): hlgs_mcmc_sample, on the GPU, reading the opacity
                           column where it lies (device memory, or the packed pinned rows of SPTCache.host)
  position_noise_(...)     train_post.py:868-878: hlgs_mcmc_noise, one pass, in place
  add_regularizers(...)    train_post.py:573-576: the opacity and scale regularisers of activate_regularized, weighted
  update_params(...)       GaussianModel._update_params (:1569-1578) through compute_relocation
  add_new_gs(...)          GaussianModel.add_new_gs (:1700-1774); its node and row writes are apply_spawn (no GPU)
  relocate_gs(...)         GaussianModel.relocate_gs (:1588-1698); its node and row writes are apply_relocation (no GPU)
  densify_round(...)       the round of train_post.py:710-767 around an SPTCache
  densify_round_nary(...)  the same round on an n-ary hierarchy (a merged scene): relocate_gs_nary over child lists,
                           its selection on the GPU (select_relocation_nary, hlgs_mcmc_select_*), its writes
                           apply_relocation_nary (no GPU); the reference has no counterpart

storage: dict name -> tensor of capacity rows for the names of spt_cache.NAMES (SPTCache.storage, or the tensors of
GaussianModel.move_storage_to, :430-460); opt_storage: dict name -> {"exp_avgs", "exp_avgs_sqs"}; nodes: capacity x 6
int32 HierarchyNode rows on the host.  Rows are written in place and nothing is reallocated.

Random numbers are the counter-based ones of csrc/hlgs_rng.h: a round is a function of (inputs, seed).  Stream 0 of the
seed samples the spawn, stream 1 the relocation; the host permutation of relocate_gs uses a torch.Generator seeded
with the seed.  Differences from the reference are listed in DESIGN.md §6 (A-25 to A-32; A-42 to A-44 for the
regularisers).
"""
import torch

from hlgs_core import _lib as L
from hlgs_core.spt_cache import NAMES

# HierarchyNode columns (types.h:60-67)
DEPTH, PARENT, CHILD_COUNT, FIRST_CHILD, NEXT_SIBLING = 0, 1, 2, 3, 4
N_MAX = 51  # utils/reloc_utils.py:4
STREAM_SPAWN, STREAM_RELOCATE = 0, 1
_EPS = torch.finfo(torch.float32).eps
_binoms = {}


def binoms(device):
    """The binomial table of utils/reloc_utils.py:5-8 on `device`."""
    import math
    key = str(device)
    if key not in _binoms:
        b = torch.zeros((N_MAX, N_MAX), dtype=torch.float32)
        for n in range(N_MAX):
            for k in range(n + 1):
                b[n, k] = math.comb(n, k)
        _binoms[key] = b.to(device)
    return _binoms[key]


def rng_uniform_host(seed, stream, first_index, n):
    """Uniform numbers first_index .. first_index + n - 1 of (seed, stream) as float64 (host code, no device)."""
    out = torch.empty((n,), dtype=torch.float64)
    L.check(L.load().hlgs_rng_uniform_host(int(seed), int(stream), int(first_index), int(n), L.ptr(out)))
    return out


def rng_fill(kind, seed, stream, first_index, n, device="cuda"):
    """The same numbers drawn on the GPU: kind "uniform64" (float64 in [0, 1)) or "normal32" (float32 N(0, 1))."""
    kinds = {"uniform64": (0, torch.float64), "normal32": (1, torch.float32)}
    code, dtype = kinds[kind]
    L.require_gpu()
    out = torch.empty((n,), dtype=dtype, device=device)
    L.check(L.load().hlgs_rng_fill(code, int(seed), int(stream), int(first_index), int(n), L.ptr(out), L.stream()))
    return out


def sample_alive(opacity, num, alive_indices=None, *, seed, stream=0, size=None, device="cuda"):
    """num draws with replacement among the candidates alive_indices (None: every row), candidate i weighing
    sigmoid(opacity[alive_indices[i], 0]).  opacity: (G, 1) float32 logits on the device or in pinned host memory,
    with any row stride (a cache.storage["opacity"] view is read in place).  Returns (sampled_idxs (num,) int32,
    counts (size,) int32 = bincount(sampled_idxs, minlength=size)) on the device; size defaults to G.  Raises
    RuntimeError where torch.multinomial does: no candidates, or a total weight of 0 or not finite."""
    lib = L.load()
    L.require_gpu()
    if opacity.dtype != torch.float32 or opacity.dim() not in (1, 2) or (opacity.dim() == 2 and opacity.shape[1] != 1):
        raise RuntimeError("opacity must be a (G, 1) float32 tensor")
    if opacity.device.type == "cpu" and not opacity.is_pinned():
        raise RuntimeError("host storage must be pinned (tensor.pin_memory()) for direct GPU access")
    G = int(opacity.shape[0])
    stride = int(opacity.stride(0)) * 4 if G > 1 else 4
    if stride < 4:
        raise RuntimeError("opacity rows must not overlap")
    size = G if size is None else int(size)
    alive = None
    n = G
    if alive_indices is not None:
        alive = alive_indices.to(device=device, dtype=torch.int32).contiguous()
        n = int(alive.numel())
        if n and (int(alive.min()) < 0 or int(alive.max()) >= G):
            raise RuntimeError("alive_indices outside the opacity rows")
    num = int(num)
    sampled = torch.empty((num,), dtype=torch.int32, device=device)
    counts = torch.empty((size,), dtype=torch.int32, device=device)
    scratch = torch.empty((lib.hlgs_mcmc_sample_scratch_size(n),), dtype=torch.uint8, device=device)
    L.check(lib.hlgs_mcmc_sample(n, opacity.data_ptr() if G else None, stride, L.ptr(alive), num, int(seed),
                                 int(stream), L.ptr(sampled), L.ptr(counts), size, L.ptr(scratch), L.stream()))
    if num:
        off = -scratch.data_ptr() % 256
        hdr = scratch[off:off + 16].cpu()  # the call's one read-back: total weight and status
        total, status = float(hdr[:8].view(torch.float64)[0]), int(hdr[8:12].view(torch.int32)[0])
        if status & 1:
            raise RuntimeError(f"sample_alive: cannot sample from {n} candidates of total weight {total} "
                               "(invalid multinomial distribution)")
        if status & 2:
            raise RuntimeError("sample_alive: a sampled row lies outside [0, size)")
    return sampled, counts


def position_noise_(means3D, opacity_raw, scaling_raw, rotation_raw, noise_lr, xyz_lr, *, seed=None, step=0,
                    noise=None, first_row=0):
    """means3D += cov @ (xi * op_sigmoid(1 - sigmoid(opacity_raw)) * noise_lr * xyz_lr) in place (train_post.py:
    868-878), for the rows from first_row on.  xi: `noise` (P, 3) when given, else the normals (3 row + c) of
    (seed, stream = step).  The tensors are the raw (unactivated) float32 device parameters."""
    lib = L.load()
    P = int(means3D.shape[0])
    ts = (means3D, opacity_raw, scaling_raw, rotation_raw) + ((noise,) if noise is not None else ())
    for t, w in zip(ts, (3, 1, 3, 4, 3)):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != P * w:
            raise RuntimeError("position_noise_ takes contiguous float32 tensors of P rows")
    L.require_gpu(*ts)
    if noise is None and seed is None:
        raise RuntimeError("position_noise_ needs a seed or the noise itself")
    L.check(lib.hlgs_mcmc_noise(P, int(first_row), L.ptr(means3D), L.ptr(opacity_raw), L.ptr(scaling_raw),
                                L.ptr(rotation_raw), L.ptr(noise), float(noise_lr) * float(xyz_lr),
                                int(seed or 0), int(step), L.stream()))
    return means3D


def add_regularizers(loss, opacity_loss, scaling_loss, lambda_opacity=0.01, lambda_scaling=0.0):
    """train_post.py:573-576: loss + lambda_opacity * opacity_loss + lambda_scaling * scaling_loss, each term only when
    its lambda is > 0 (the defaults are the reference's, :74-75), so that with lambda_scaling = 0 an overflowed
    scaling_loss (inf) cannot turn the loss into NaN through 0 * inf; with both lambdas 0 `loss` itself is returned.
    opacity_loss and scaling_loss are the last two results of hlgs_core.activations.activate_regularized; they are also
    what train_post.py:659-660 logs: "Mean Opacity" = opacity_loss and "Mean Scaling" = scaling_loss / 3."""
    if lambda_opacity > 0:
        loss = loss + lambda_opacity * opacity_loss
    if lambda_scaling > 0:
        loss = loss + lambda_scaling * scaling_loss
    return loss


def _inverse_sigmoid(x):
    return torch.log(x / (1 - x))


def update_params(storage, idxs, ratio, device="cuda"):
    """GaussianModel._update_params (:1569-1578) for the rows idxs (int64, host): the relocated opacity and scale of a
    Gaussian drawn ratio[idx] times, unactivated again.  Returns the reference's six values (xyz, f_dc, f_rest,
    new_opacity (n, 1), new_scaling (n, 3), rotation); the two new ones are device tensors.  N = ratio + 1 is capped at
    N_MAX, the size of the binomial table (the reference reads past it, A-27)."""
    from hlgs_core.raster import compute_relocation
    idxs = idxs.to("cpu", torch.int64)
    op = torch.sigmoid(storage["opacity"][idxs, 0].to(device))
    sc = torch.exp(storage["scaling"][idxs].to(device))
    N = (ratio.to(device)[idxs.to(device)].reshape(-1).to(torch.int32) + 1).clamp_(max=N_MAX)
    new_op, new_sc = compute_relocation(op, sc, N, binoms(device), N_MAX)
    new_op = torch.clamp(new_op.unsqueeze(-1), max=1.0 - _EPS, min=0.005)
    return (storage["xyz"][idxs], storage["f_dc"][idxs], storage["f_rest"][idxs], _inverse_sigmoid(new_op),
            torch.log(new_sc.reshape(-1, 3)), storage["rotation"][idxs])


def _opacity_column(storage, size, device):
    """The opacity logits of the first `size` rows on the device.  Host storage is copied (one torch copy of the
    column) rather than sampled in place: the sampler's strided read of packed host rows costs a 64-byte line over the
    host link per 4 useful bytes (157 ms against 60 ms with the copy at 50M rows, 31 against 37 ms at 10M)."""
    op = storage["opacity"][:size]
    return op if op.device.type != "cpu" else op.to(device)


def _leaves(nodes, size):
    return torch.where(nodes[:size, CHILD_COUNT] == 0)[0]


def apply_spawn(nodes, storage, add_idx, rows, size):
    """The writes of add_new_gs (:1732-1767), no GPU: every node of add_idx (int64, ascending) becomes the parent of two
    new leaves at size + 2 k and size + 2 k + 1, both holding `rows` [k] = (xyz, f_dc, f_rest, opacity, scaling,
    rotation) of update_params.  Returns the new size."""
    add_idx = add_idx.to("cpu", torch.int64)
    n = int(add_idx.numel())
    if size + 2 * n > nodes.shape[0] or size + 2 * n > storage["xyz"].shape[0]:
        raise RuntimeError(f"add_new_gs: {2 * n} new rows do not fit the capacity ({nodes.shape[0]} node rows, "
                           f"{storage['xyz'].shape[0]} storage rows, size {size})")
    if n == 0:
        return size
    first = torch.arange(0, n, dtype=torch.int32) * 2 + size
    nodes[add_idx, CHILD_COUNT] = 2
    nodes[add_idx, FIRST_CHILD] = first
    new_nodes = torch.zeros((2 * n, 6), dtype=torch.int32)
    new_nodes[0::2, DEPTH] = nodes[add_idx, DEPTH] + 1
    new_nodes[0::2, PARENT] = add_idx.to(torch.int32)
    new_nodes[0::2, NEXT_SIBLING] = first + 1
    new_nodes[1::2, DEPTH] = nodes[add_idx, DEPTH] + 1
    new_nodes[1::2, PARENT] = add_idx.to(torch.int32)
    nodes[size:size + 2 * n] = new_nodes
    for k, v in zip(("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation"), rows):
        storage[k][size:size + 2 * n] = v.to("cpu").repeat_interleave(2, dim=0)
    return size + 2 * n


def add_new_gs(storage, nodes, size, cap_max, *, seed, device="cuda"):
    """GaussianModel.add_new_gs (:1700-1774): with the target size min(cap_max, int(1.05 size)), draw leaves by
    opacity, keep the ones drawn exactly once, and give each two children (appended at size...) holding the relocated
    opacity and scale of N = 2.  A kept leaf adds two rows, so (target - size) // 2 leaves are drawn and the new size
    stays within the target; the reference draws target - size of them and can pass its target, and with it cap_max,
    the capacity of its storage, by as much again (A-28).  Returns the new size (the reference returns the number of
    draws and adds the rows to self.size)."""
    size = int(size)
    num_gs = max(0, min(int(cap_max), int(1.05 * size)) - size) // 2
    if num_gs <= 0:
        return size
    alive = _leaves(nodes, size)
    _, counts = sample_alive(_opacity_column(storage, size, device), num_gs, alive, seed=seed, stream=STREAM_SPAWN,
                             size=size, device=device)
    add_idx = torch.where(counts == 1)[0].cpu()
    ratio = torch.ones((size,), dtype=torch.int32)  # ratio[add_idx] = 1: every kept row relocates with N = 2
    return apply_spawn(nodes, storage, add_idx, update_params(storage, add_idx, ratio, device), size)


def select_relocation(nodes, dead_mask, size):
    """The selection of relocate_gs before it samples (:1591-1610), no GPU: (dead_indices after the sibling
    exclusion, their sibling_indices, the candidate leaves alive_indices)."""
    dead_mask = dead_mask[:size]
    dead = dead_mask.nonzero(as_tuple=True)[0]
    alive_mask = torch.logical_and(~dead_mask, nodes[:size, CHILD_COUNT] == 0)
    alive = alive_mask.nonzero(as_tuple=True)[0]
    # if a node and its sibling want to die, one of them stays (:1597-1599)
    dead = dead[~torch.isin(dead, nodes[dead, NEXT_SIBLING].long())]
    first_child = nodes[dead, NEXT_SIBLING] > 0
    sibling = torch.zeros_like(dead, dtype=torch.int32)
    sibling[first_child] = nodes[dead[first_child], NEXT_SIBLING]
    sibling[~first_child] = nodes[nodes[dead[~first_child], PARENT].long(), FIRST_CHILD]
    alive = alive[~torch.isin(alive, sibling.long())]
    return dead, sibling, alive


def apply_relocation(nodes, storage, opt_storage, dead_indices, sibling_indices, reinit_idx, new_opacity, new_scaling,
                     skybox_points, size):
    """The writes of relocate_gs (:1627-1698), no GPU, in the reference's statement order: the dead rows take the
    parameters of the leaves they respawn at (with the relocated opacity and scale); each dead leaf's sibling is
    promoted into their parent, deepest first; the leaf reinit_idx[k] becomes the parent of dead_indices[k] and
    sibling_indices[k]; the sibling row is a copy of the dead row (without f_rest and rotation, A-25) with zeroed
    moments.  Index tensors are host tensors of one length."""
    dead = dead_indices.to("cpu", torch.int64)
    sib = sibling_indices.to("cpu", torch.int64)
    re = reinit_idx.to("cpu", torch.int64)
    if dead.numel() == 0:
        return
    s = storage
    s["xyz"][dead] = s["xyz"][re]
    s["f_dc"][dead] = s["f_dc"][re]
    s["f_rest"][dead] = s["f_rest"][re]
    s["rotation"][dead] = s["rotation"][re]
    s["opacity"][dead] = new_opacity.to("cpu")
    s["scaling"][dead] = new_scaling.to("cpu")
    # the not-dead sibling moves into the parent (:1641-1664)
    parent = nodes[dead, PARENT].long()
    for depth in range(int(torch.max(nodes[skybox_points:size, DEPTH])), 0, -1):
        m = nodes[sib, DEPTH] == depth
        sd, pd = sib[m], parent[m]
        for k in NAMES:
            s[k][pd] = s[k][sd]
        nodes[pd, CHILD_COUNT] = nodes[sd, CHILD_COUNT]
        nodes[pd, FIRST_CHILD] = nodes[sd, FIRST_CHILD]
        # the sibling's children move up; a leaf sibling has none (the reference re-parents row 0 there, A-26)
        inner = nodes[sd, CHILD_COUNT] > 0
        sd, pd = sd[inner], pd[inner]
        c1 = nodes[sd, FIRST_CHILD].long()
        nodes[c1, PARENT] = pd.to(torch.int32)
        nodes[c1, DEPTH] = nodes[pd, DEPTH] + 1
        c2 = nodes[c1, NEXT_SIBLING].long()
        nodes[c2, PARENT] = pd.to(torch.int32)
        nodes[c2, DEPTH] = nodes[pd, DEPTH] + 1
    # the respawn leaves now have two children: the dead node and its former sibling (:1667-1682)
    nodes[re, CHILD_COUNT] = 2
    nodes[re, FIRST_CHILD] = dead.to(torch.int32)
    for rows, nxt in ((dead, sib.to(torch.int32)), (sib, 0)):
        nodes[rows, DEPTH] = nodes[re, DEPTH] + 1
        nodes[rows, PARENT] = re.to(torch.int32)
        nodes[rows, CHILD_COUNT] = 0
        nodes[rows, FIRST_CHILD] = 0
        nodes[rows, NEXT_SIBLING] = nxt
    # the sibling is a copy (:1684-1689: xyz, opacity, f_dc, scaling)
    for k in ("xyz", "opacity", "f_dc", "scaling"):
        s[k][sib] = s[k][dead]
    for k in NAMES:
        opt_storage[k]["exp_avgs"][sib] = 0
        opt_storage[k]["exp_avgs_sqs"][sib] = 0


def relocate_gs(storage, opt_storage, nodes, dead_mask, size, skybox_points, *, seed, device="cuda"):
    """GaussianModel.relocate_gs (:1588-1698): the dead leaves of dead_mask (host bool, size entries) respawn as
    children of leaves drawn by opacity.  Returns the number of relocated Gaussians."""
    size = int(size)
    dead_mask = dead_mask.to("cpu")
    if int(dead_mask.sum()) == 0:
        return 0
    dead, sibling, alive = select_relocation(nodes, dead_mask, size)
    reinit, counts = sample_alive(_opacity_column(storage, size, device), 2 * int(dead.numel()), alive, seed=seed,
                                  stream=STREAM_RELOCATE, size=size, device=device)
    reinit = reinit.unique().cpu().long()
    g = torch.Generator()
    g.manual_seed(int(seed) & 0x7fffffffffffffff)
    reinit = reinit[torch.randperm(len(reinit), generator=g)[:len(dead)]]
    if len(reinit) < len(dead):  # fewer distinct respawn places than dead Gaussians (:1622-1625)
        dead, sibling = dead[:len(reinit)], sibling[:len(reinit)]
    _, _, _, new_opacity, new_scaling, _ = update_params(storage, reinit, counts, device)
    apply_relocation(nodes, storage, opt_storage, dead, sibling, reinit, new_opacity, new_scaling, skybox_points, size)
    return int(dead.numel())


def densify_round(cache, nodes, size, *, cap_max, seed, spt_args, min_opacity=0.005, device="cuda",
                  spt_on_device=False):
    """One densification round of train_post.py:710-767 around an SPTCache whose storage has spare capacity: the
    cache is emptied into storage (cache.reset), leaves are spawned (add_new_gs), the leaves that were at or below
    min_opacity before the spawn are relocated (relocate_gs), the SPTs are rebuilt and handed to the cache
    (cache.reset(spt)).  spt_args: the keyword arguments of build_hierarchical_spt after `root` (SPT_Root_Volume,
    target_granularity, ...); root defaults to the skybox size.  spt_on_device: rebuild with
    build_hierarchical_spt_device, which reads nodes[:new_size] and the storage views where they lie (no host copy of
    the parameter columns) and leaves the SPT arrays on the device; otherwise the host build.  Returns the new size."""
    from hlgs_core.spt import build_hierarchical_spt, build_hierarchical_spt_device
    if getattr(cache, "nary", False):  # select_relocation / apply_relocation assume sibling pairs
        raise ValueError("densify_round: the MCMC round needs a binary hierarchy; this cache streams an n-ary one")
    size = int(size)
    cache.reset()
    storage, opt_storage = cache.storage, cache.opt_storage
    threshold = _inverse_sigmoid(torch.tensor(min_opacity)).item()
    dead_indices = torch.where(storage["opacity"][:size, 0] <= threshold)[0]
    new_size = add_new_gs(storage, nodes, size, cap_max, seed=seed, device=device)
    # newly spawned Gaussians are not dead, and only leaves are redistributed (:749-763)
    dead_mask = torch.zeros(new_size, dtype=torch.bool)
    dead_mask[dead_indices] = True
    dead_mask = torch.logical_and(dead_mask, nodes[:new_size, CHILD_COUNT] == 0)
    relocate_gs(storage, opt_storage, nodes, dead_mask, new_size, cache.sky, seed=seed, device=device)
    args = dict(spt_args)
    root = args.pop("root", cache.sky)
    if spt_on_device:
        spt = build_hierarchical_spt_device(nodes[:new_size], storage["xyz"][:new_size], storage["scaling"][:new_size],
                                            root, **args, device=device)
    else:
        spt = build_hierarchical_spt(nodes[:new_size], storage["xyz"][:new_size], storage["scaling"][:new_size], root,
                                     **args)
    cache.reset(spt)
    return new_size


# ---------------------------------------------------------------------------------------------------------------
# The round on an n-ary hierarchy (a merged scene: child lists of any length, include/hlgs.h "n-ary relocation").
# The entry points above stay the binary path; these stand beside them and, on a hierarchy the binary path accepts,
# leave its result bit for bit.  add_new_gs and apply_spawn need no n-ary form: they read child_count == 0, overwrite
# first_child (a merged leaf holds id + 1 there, which nothing reads) and append pairs, which are legal lists.
def select_relocation_nary(nodes, dead_mask, size, sky, device="cuda"):
    """The selection of the n-ary relocation (hlgs_mcmc_select_count / _emit, csrc/mcmc_nary.hip): uploads
    nodes[:size] and the flags, counts, reads the four sizes back (the call's one read-back) and emits.  Returns
    (group_parent, group_survivor, group_start, free_rows, alive), int32 tensors on the device: per kept group its
    parent, its promoted survivor (-1 for an unlink group) and its freed rows free_rows[group_start[g] :
    group_start[g + 1]], groups ascending by first freed row; alive: the respawn candidates, ascending.  A child list
    that breaks the n-ary contract raises RuntimeError.  With size 0 or no flag set nothing is launched, the table is
    not read, and every list is empty -- alive too, which then does not mean "no leaves"; flags that select no group
    still return the candidates."""
    lib = L.load()
    L.require_gpu()
    size, sky = int(size), int(sky)
    i32 = dict(dtype=torch.int32, device=device)
    flags = dead_mask[:size].to(torch.uint8)
    if nodes.shape[0] < size or flags.numel() != size:
        raise RuntimeError("select_relocation_nary: nodes and dead_mask must hold `size` rows")
    if size == 0 or not bool(flags.any()):  # nothing to relocate: no launch (relocate_gs returns before it selects)
        return tuple(torch.zeros(n, **i32) for n in (0, 0, 1, 0, 0))
    nd = nodes[:size].to(device=device, dtype=torch.int32).contiguous()
    flags = flags.to(device).contiguous()
    scratch = torch.empty((lib.hlgs_mcmc_select_scratch_size(size) + 256,), dtype=torch.uint8, device=device)
    base = scratch[-scratch.data_ptr() % 256:]
    counts = torch.empty((4,), **i32)
    L.check(lib.hlgs_mcmc_select_count(size, sky, L.ptr(nd), L.ptr(flags), L.ptr(base), L.ptr(counts), L.stream()))
    n_groups, n_free, n_alive, status = counts.tolist()
    if status:
        raise RuntimeError("select_relocation_nary: a child list breaks the n-ary contract (a link out of range, a "
                           "list shorter or longer than child_count, or a row in another row's list)")
    gp, gs = torch.empty((n_groups,), **i32), torch.empty((n_groups,), **i32)
    start = torch.zeros((n_groups + 1,), **i32)
    free, alive = torch.empty((n_free,), **i32), torch.empty((n_alive,), **i32)
    L.check(lib.hlgs_mcmc_select_emit(size, sky, L.ptr(nd), L.ptr(flags), L.ptr(base), L.ptr(gp), L.ptr(gs),
                                      L.ptr(start), L.ptr(free), L.ptr(alive), L.stream()))
    return gp, gs, start, free, alive


def apply_relocation_nary(nodes, storage, opt_storage, group_parent, group_survivor, group_start, free_rows,
                          reinit_idx, new_opacity, new_scaling, skybox_points, size):
    """The writes of the n-ary relocation, no GPU, over the changed rows only; group g (select_relocation_nary's lists,
    cut to the groups that found a place) respawns at the leaf reinit_idx[g], whose relocated opacity and scale are
    new_opacity[g], new_scaling[g].  In this order: (1) every dead member takes the parameters of its group's place;
    (2) unlink groups: the parent's list is rewritten to its survivors in their old order -- before the promotions,
    because an unlink parent can be the survivor of a promote group one level up; (3) promote groups, deepest survivor
    first (:1641-1664): the parent takes the survivor's six rows, child_count and first_child, and every child of the
    survivor its new parent and depth (A-26, A-29 as in apply_relocation); (4) the place becomes the parent of the
    group's freed rows, chained in order; (5) a promoted survivor's row is a copy of the group's first freed row
    (A-25) with zeroed moments.  On a binary hierarchy this is apply_relocation, statement for statement."""
    re = reinit_idx.to("cpu", torch.int64)
    n = int(re.numel())
    if n == 0:
        return
    if n > int(group_parent.numel()):
        raise RuntimeError("apply_relocation_nary: more respawn places than groups")
    # the first n groups are placed; longer lists (fewer places than groups) are cut here
    gp = group_parent.to("cpu", torch.int64)[:n]
    gs = group_survivor.to("cpu", torch.int64)[:n]
    st = group_start.to("cpu", torch.int64)[:n + 1]
    fr = free_rows.to("cpu", torch.int64)[:int(st[n])]
    m = st[1:n + 1] - st[:n]
    promote = gs >= 0
    k = m - promote.long()
    gid = torch.repeat_interleave(torch.arange(n), m)
    pos = torch.arange(int(fr.numel())) - st[gid]
    is_dead = pos < k[gid]  # in a promote group the last freed row is the survivor
    dead, dead_re = fr[is_dead], re[gid[is_dead]]
    s = storage
    s["xyz"][dead] = s["xyz"][dead_re]
    s["f_dc"][dead] = s["f_dc"][dead_re]
    s["f_rest"][dead] = s["f_rest"][dead_re]
    s["rotation"][dead] = s["rotation"][dead_re]
    s["opacity"][dead] = new_opacity.to("cpu")[gid[is_dead]]
    s["scaling"][dead] = new_scaling.to("cpu")[gid[is_dead]]
    # unlink groups: the parent keeps its survivors, in their old order (one pass per rank of the longest list)
    up = gp[~promote]
    if up.numel():
        cc = nodes[up, CHILD_COUNT].long()
        cur = nodes[up, FIRST_CHILD].long()
        prev = torch.full_like(cur, -1)
        for j in range(int(cc.max())):
            act = j < cc
            keep = act & ~torch.isin(cur, dead)
            head, link = keep & (prev < 0), keep & (prev >= 0)
            nodes[up[head], FIRST_CHILD] = cur[head].to(torch.int32)
            nodes[prev[link], NEXT_SIBLING] = cur[link].to(torch.int32)
            prev = torch.where(keep, cur, prev)
            cur = torch.where(act, nodes[cur, NEXT_SIBLING].long(), cur)
        nodes[prev, NEXT_SIBLING] = 0
        nodes[up, CHILD_COUNT] = (cc - k[~promote]).to(torch.int32)
    # promote groups: the survivor moves into the parent (:1641-1664), deepest first
    sv, pv = gs[promote], gp[promote]
    for depth in range(int(torch.max(nodes[skybox_points:size, DEPTH])) if sv.numel() else 0, 0, -1):
        lv = nodes[sv, DEPTH] == depth
        sd, pd = sv[lv], pv[lv]
        for name in NAMES:
            s[name][pd] = s[name][sd]
        nodes[pd, CHILD_COUNT] = nodes[sd, CHILD_COUNT]
        nodes[pd, FIRST_CHILD] = nodes[sd, FIRST_CHILD]
        # the survivor's children move up, the whole list; a leaf survivor has none (A-26)
        inner = nodes[sd, CHILD_COUNT] > 0
        sd, pd = sd[inner], pd[inner]
        if sd.numel() == 0:
            continue
        cc = nodes[sd, CHILD_COUNT].long()
        cur = nodes[sd, FIRST_CHILD].long()
        for j in range(int(cc.max())):
            act = j < cc
            ca, pa = cur[act], pd[act]
            nodes[ca, PARENT] = pa.to(torch.int32)
            nodes[ca, DEPTH] = nodes[pa, DEPTH] + 1
            cur = torch.where(act, nodes[cur, NEXT_SIBLING].long(), cur)
    # the respawn leaves become the parents of their groups' freed rows (:1667-1682)
    nodes[re, CHILD_COUNT] = m.to(torch.int32)
    nodes[re, FIRST_CHILD] = fr[st[:n]].to(torch.int32)
    place = re[gid]
    nxt = torch.zeros_like(fr)
    nxt[:-1] = fr[1:]
    nxt[pos == m[gid] - 1] = 0
    nodes[fr, DEPTH] = nodes[place, DEPTH] + 1
    nodes[fr, PARENT] = place.to(torch.int32)
    nodes[fr, CHILD_COUNT] = 0
    nodes[fr, FIRST_CHILD] = 0
    nodes[fr, NEXT_SIBLING] = nxt.to(torch.int32)
    # a promoted survivor's row is a copy of the first freed row (:1684-1689: xyz, opacity, f_dc, scaling)
    first = fr[st[:n]][promote]
    for name in ("xyz", "opacity", "f_dc", "scaling"):
        s[name][sv] = s[name][first]
    for name in NAMES:
        opt_storage[name]["exp_avgs"][sv] = 0
        opt_storage[name]["exp_avgs_sqs"][sv] = 0


def relocate_gs_nary(storage, opt_storage, nodes, dead_mask, size, skybox_points, *, seed, device="cuda"):
    """relocate_gs on an n-ary hierarchy: the groups of select_relocation_nary respawn as the children of leaves drawn
    by opacity, one place per group (2 n_groups draws on STREAM_RELOCATE, unique, the seeded permutation; with fewer
    places than groups the first len(places) groups are kept).  Returns the number of dead Gaussians relocated.  On a
    binary hierarchy the state and the count are relocate_gs's, bit for bit."""
    size = int(size)
    dead_mask = dead_mask.to("cpu")
    if int(dead_mask.sum()) == 0:
        return 0
    gp, gs, start, free, alive = select_relocation_nary(nodes, dead_mask, size, skybox_points, device)
    n_groups = int(gp.numel())
    if n_groups == 0:  # flags on rows that are no candidates, or only single dead children of wide lists
        return 0
    # the candidates stay on the device: they are the one list of the selection that scales with the scene
    reinit, counts = sample_alive(_opacity_column(storage, size, device), 2 * n_groups, alive, seed=seed,
                                  stream=STREAM_RELOCATE, size=size, device=device)
    reinit = reinit.unique().cpu().long()
    g = torch.Generator()
    g.manual_seed(int(seed) & 0x7fffffffffffffff)
    reinit = reinit[torch.randperm(len(reinit), generator=g)[:n_groups]]
    n = min(n_groups, len(reinit))  # fewer distinct respawn places than groups (:1622-1625)
    gp, gs, start = gp[:n].cpu(), gs[:n].cpu(), start[:n + 1].cpu()
    _, _, _, new_opacity, new_scaling, _ = update_params(storage, reinit, counts, device)
    apply_relocation_nary(nodes, storage, opt_storage, gp, gs, start, free.cpu(), reinit, new_opacity, new_scaling,
                          skybox_points, size)
    return int(start[n]) - int((gs >= 0).sum())


def densify_round_nary(cache, nodes, size, *, cap_max, seed, spt_args, min_opacity=0.005, device="cuda",
                       spt_on_device=False):
    """densify_round for a cache over an n-ary hierarchy (a merged scene), with the same arguments and sequence: the
    cache is emptied, leaves are spawned (add_new_gs as it is: it reads child_count == 0 and appends pairs), the
    leaves at or below min_opacity before the spawn are relocated by relocate_gs_nary, the SPTs are rebuilt with the
    n-ary build when the cache streams an n-ary hierarchy, and handed to the cache.  A binary cache is accepted too:
    the round is then densify_round's, bit for bit.  Returns the new size."""
    from hlgs_core.spt import build_hierarchical_spt, build_hierarchical_spt_device
    size = int(size)
    nary = bool(getattr(cache, "nary", False))
    cache.reset()
    storage, opt_storage = cache.storage, cache.opt_storage
    threshold = _inverse_sigmoid(torch.tensor(min_opacity)).item()
    dead_indices = torch.where(storage["opacity"][:size, 0] <= threshold)[0]
    new_size = add_new_gs(storage, nodes, size, cap_max, seed=seed, device=device)
    dead_mask = torch.zeros(new_size, dtype=torch.bool)
    dead_mask[dead_indices] = True
    dead_mask = torch.logical_and(dead_mask, nodes[:new_size, CHILD_COUNT] == 0)
    relocate_gs_nary(storage, opt_storage, nodes, dead_mask, new_size, cache.sky, seed=seed, device=device)
    args = dict(spt_args)
    root = args.pop("root", cache.sky)
    build = build_hierarchical_spt_device if spt_on_device else build_hierarchical_spt
    if spt_on_device:
        args["device"] = device
    spt = build(nodes[:new_size], storage["xyz"][:new_size], storage["scaling"][:new_size], root, **args, nary=nary)
    cache.reset(spt)
    return new_size
