"""Reference code shared by tests/test_mcmc_cpu.py and tests/test_gpu_mcmc.py: a pure-Python Philox4x32-10 with the
number mappings of csrc/hlgs_rng.h, scalar (loop-per-node) restatements of the hierarchy writes of
GaussianModel.add_new_gs / relocate_gs (scene/gaussian_model.py:1588-1774), the link invariants of a dynamic
hierarchy, and the position noise of train_post.py:868-878 in torch at a chosen precision."""
import numpy as np
import torch

DEPTH, PARENT, CHILD_COUNT, FIRST_CHILD, NEXT_SIBLING = 0, 1, 2, 3, 4
NAMES = ("xyz", "f_dc", "opacity", "scaling", "rotation", "f_rest")
SHAPES = {"xyz": (3,), "f_dc": (1, 3), "opacity": (1,), "scaling": (3,), "rotation": (4,), "f_rest": (3, 3)}
M32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def rng_words(seed, stream, index):
    return philox4x32_10((index & M32, index >> 32, stream, 0), (seed & M32, seed >> 32))


def uniform53(seed, stream, index):
    w = rng_words(seed, stream, index)
    return float(((w[0] >> 5) << 26) + (w[1] >> 6)) * 2.0 ** -53


def uniforms(seed, stream, first, n):
    return np.array([uniform53(seed, stream, first + i) for i in range(n)], np.float64)


# ------------------------------------------------------------------ hierarchy writes, one node at a time
def make_storage(cap, rng):
    storage = {k: torch.tensor(rng.normal(size=(cap,) + SHAPES[k]).astype(np.float32)) for k in NAMES}
    opt = {k: {m: torch.tensor(rng.normal(size=(cap,) + SHAPES[k]).astype(np.float32))
               for m in ("exp_avgs", "exp_avgs_sqs")} for k in NAMES}
    return storage, opt


def clone_state(nodes, storage, opt):
    return (nodes.clone(), {k: v.clone() for k, v in storage.items()},
            {k: {m: t.clone() for m, t in v.items()} for k, v in opt.items()})


def spawn_ref(nodes, storage, add_idx, rows, size):
    """add_new_gs (:1732-1767) per kept row."""
    for k, a in enumerate(int(a) for a in add_idx):
        c = size + 2 * k
        nodes[a, CHILD_COUNT] = 2
        nodes[a, FIRST_CHILD] = c
        d = int(nodes[a, DEPTH]) + 1
        nodes[c] = torch.tensor([d, a, 0, 0, c + 1, 0], dtype=torch.int32)
        nodes[c + 1] = torch.tensor([d, a, 0, 0, 0, 0], dtype=torch.int32)
        for name, v in zip(("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation"), rows):
            storage[name][c] = v[k]
            storage[name][c + 1] = v[k]
    return size + 2 * len(add_idx)


def select_ref(nodes, dead_mask, size):
    """relocate_gs :1591-1610 per node."""
    dead_all = [i for i in range(size) if dead_mask[i]]
    excluded = {int(nodes[d, NEXT_SIBLING]) for d in dead_all}
    dead = [d for d in dead_all if d not in excluded]
    sib = []
    for d in dead:
        ns = int(nodes[d, NEXT_SIBLING])
        sib.append(ns if ns > 0 else int(nodes[int(nodes[d, PARENT]), FIRST_CHILD]))
    alive = [i for i in range(size) if not dead_mask[i] and nodes[i, CHILD_COUNT] == 0 and i not in set(sib)]
    return dead, sib, alive


def relocation_ref(nodes, storage, opt, dead, sib, re, new_opacity, new_scaling, sky, size):
    """relocate_gs :1627-1698 per node, in the statement order of the reference; the children of a promoted sibling
    are re-parented only where it has children."""
    dead, sib, re = [int(v) for v in dead], [int(v) for v in sib], [int(v) for v in re]
    n = len(dead)
    for k in range(n):
        for name in ("xyz", "f_dc", "f_rest", "rotation"):
            storage[name][dead[k]] = storage[name][re[k]]
    for k in range(n):
        storage["opacity"][dead[k]] = new_opacity[k]
        storage["scaling"][dead[k]] = new_scaling[k]
    parent = [int(nodes[d, PARENT]) for d in dead]
    for depth in range(max(int(nodes[i, DEPTH]) for i in range(sky, size)), 0, -1):
        level = [k for k in range(n) if int(nodes[sib[k], DEPTH]) == depth]
        for k in level:
            s, p = sib[k], parent[k]
            for name in NAMES:
                storage[name][p] = storage[name][s]
            nodes[p, CHILD_COUNT] = nodes[s, CHILD_COUNT]
            nodes[p, FIRST_CHILD] = nodes[s, FIRST_CHILD]
            if int(nodes[s, CHILD_COUNT]) > 0:
                c1 = int(nodes[s, FIRST_CHILD])
                c2 = int(nodes[c1, NEXT_SIBLING])
                for c in (c1, c2):
                    nodes[c, PARENT] = p
                    nodes[c, DEPTH] = int(nodes[p, DEPTH]) + 1
    for k in range(n):
        nodes[re[k], CHILD_COUNT] = 2
        nodes[re[k], FIRST_CHILD] = dead[k]
    for k in range(n):
        nodes[dead[k]] = torch.tensor([int(nodes[re[k], DEPTH]) + 1, re[k], 0, 0, sib[k], int(nodes[dead[k], 5])],
                                      dtype=torch.int32)
    for k in range(n):
        nodes[sib[k]] = torch.tensor([int(nodes[re[k], DEPTH]) + 1, re[k], 0, 0, 0, int(nodes[sib[k], 5])],
                                     dtype=torch.int32)
    for k in range(n):
        for name in ("xyz", "opacity", "f_dc", "scaling"):
            storage[name][sib[k]] = storage[name][dead[k]]
    for k in range(n):
        for name in NAMES:
            opt[name]["exp_avgs"][sib[k]] = 0
            opt[name]["exp_avgs_sqs"][sib[k]] = 0


def leaf_count(nodes, sky, size):
    return int((nodes[sky:size, CHILD_COUNT] == 0).sum())


def check_links(nodes, sky, size, root=None):
    """The link invariants of a dynamic hierarchy over rows [sky, size): every node with two children has a first
    child and, through its next_sibling, a second child inside the range whose parent fields point back, the second
    child's next_sibling is 0, and every node but the root is the child of some node.  (Depth is not checked: the
    reference leaves the depth of a promoted node's grandchildren stale.)"""
    nd = np.asarray(nodes[:size].cpu().numpy(), np.int64)
    root = sky if root is None else root
    cc = nd[sky:, CHILD_COUNT]
    assert set(np.unique(cc).tolist()) <= {0, 2}, np.unique(cc)
    inner = np.where(nd[:, CHILD_COUNT] == 2)[0]
    inner = inner[inner >= sky]
    c1 = nd[inner, FIRST_CHILD]
    assert ((c1 >= sky) & (c1 < size)).all()
    c2 = nd[c1, NEXT_SIBLING]
    assert ((c2 >= sky) & (c2 < size)).all()
    assert (c1 != c2).all()
    np.testing.assert_array_equal(nd[c1, PARENT], inner)
    np.testing.assert_array_equal(nd[c2, PARENT], inner)
    assert (nd[c2, NEXT_SIBLING] == 0).all()
    children = np.concatenate([c1, c2])
    assert len(np.unique(children)) == len(children)
    np.testing.assert_array_equal(np.sort(children), np.setdiff1d(np.arange(sky, size), [root]))


# ------------------------------------------------------------------ position noise (train_post.py:868-878)
def build_rotation(r):
    """utils/general_utils.py:82-103"""
    norm = torch.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2] + r[:, 3] * r[:, 3])
    q = r / norm[:, None]
    R = torch.zeros((q.size(0), 3, 3), dtype=r.dtype, device=r.device)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R[:, 0, 0] = 1 - 2 * (y * y + z * z)
    R[:, 0, 1] = 2 * (x * y - r * z)
    R[:, 0, 2] = 2 * (x * z + r * y)
    R[:, 1, 0] = 2 * (x * y + r * z)
    R[:, 1, 1] = 1 - 2 * (x * x + z * z)
    R[:, 1, 2] = 2 * (y * z - r * x)
    R[:, 2, 0] = 2 * (x * z - r * y)
    R[:, 2, 1] = 2 * (y * z + r * x)
    R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def noise_delta(opacity, scales, rotations, xi, noise_lr, xyz_lr, dtype):
    """The increment of train_post.py:870-878 composed of torch ops as the reference composes them, at `dtype`, from
    the float32 inputs: what is added to means3D."""
    opacity, scales, rotations, xi = (t.to(dtype) for t in (opacity, scales, rotations, xi))

    def op_sigmoid(x, k=100, x0=0.995):
        return 1 / (1 + torch.exp(-k * (x - x0)))
    s = torch.exp(scales)
    L = torch.zeros((s.shape[0], 3, 3), dtype=dtype, device=s.device)
    L[:, 0, 0], L[:, 1, 1], L[:, 2, 2] = s[:, 0], s[:, 1], s[:, 2]
    L = build_rotation(torch.nn.functional.normalize(rotations)) @ L
    cov = L @ L.transpose(1, 2)
    noise = xi * op_sigmoid(1 - torch.sigmoid(opacity)) * noise_lr * xyz_lr
    return torch.bmm(cov, noise.unsqueeze(-1)).squeeze(-1)
