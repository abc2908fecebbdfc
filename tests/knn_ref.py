"""The restatement simple_knn.distCUDA2 is tested against, and the seeded scenes it is tested on.

knn_ref(xyz, device) evaluates the contract (include/hlgs.h, hlgs_knn_mean_dist2) over all pairs in float32 with
separate eager torch operations, so every product and sum is rounded on its own: d = dx*dx; d = d + dy*dy;
d = d + dz*dz; the self index set to +inf; the three smallest by torch.topk; ((b0 + b1) + b2) / 3.  It runs unchanged
on the CPU and on the GPU.  knn_ref_numpy is the same in numpy (the two agree bit for bit, tests/test_knn_cpu.py) and
knn_f64 the same definition in float64 (scipy's cKDTree when scipy imports, numpy all-pairs otherwise).
"""
import numpy as np
import torch

CHUNK = 1024  # rows of the all-pairs matrix evaluated at a time


def knn_ref(xyz, device="cpu"):
    """(P, 3) array or tensor -> (P,) float32 tensor on `device`."""
    p = torch.as_tensor(xyz).to(device=device, dtype=torch.float32).contiguous()
    P = p.shape[0]
    out = torch.empty(P, dtype=torch.float32, device=device)
    x, y, z = p[:, 0].contiguous(), p[:, 1].contiguous(), p[:, 2].contiguous()
    cols = torch.arange(P, device=device)
    # a tensor divisor: torch divides by a Python scalar on the GPU as a product with its reciprocal, which is not the
    # correctly rounded quotient the contract asks for
    three = torch.full((1,), 3.0, dtype=torch.float32, device=device)
    for r0 in range(0, P, CHUNK):
        r1 = min(P, r0 + CHUNK)
        dx = x[None, :] - x[r0:r1, None]
        dy = y[None, :] - y[r0:r1, None]
        dz = z[None, :] - z[r0:r1, None]
        d = dx * dx
        d = d + dy * dy
        d = d + dz * dz
        d[cols[r0:r1] - r0, cols[r0:r1]] = float("inf")
        if P < 3:  # fewer columns than neighbours: the missing ones count as +inf
            d = torch.cat((d, torch.full((r1 - r0, 3 - P), float("inf"), device=device)), dim=1)
        b = torch.topk(d, 3, dim=1, largest=False, sorted=True)[0]
        out[r0:r1] = ((b[:, 0] + b[:, 1]) + b[:, 2]) / three
    return out


def _three_smallest(d):
    if d.shape[1] < 3:
        d = np.concatenate((d, np.full((d.shape[0], 3 - d.shape[1]), np.inf, d.dtype)), axis=1)
    return np.sort(np.partition(d, 2, axis=1)[:, :3], axis=1)


def knn_ref_numpy(xyz, dtype=np.float32):
    """The restatement in numpy, in `dtype` (float32: the contract; float64: its exact-arithmetic yardstick)."""
    p = np.ascontiguousarray(xyz, dtype=dtype)
    P = p.shape[0]
    out = np.empty(P, dtype)
    three = dtype(3)
    for r0 in range(0, P, CHUNK):
        r1 = min(P, r0 + CHUNK)
        dx = p[None, :, 0] - p[r0:r1, None, 0]
        dy = p[None, :, 1] - p[r0:r1, None, 1]
        dz = p[None, :, 2] - p[r0:r1, None, 2]
        d = dx * dx
        d = d + dy * dy
        d = d + dz * dz
        d[np.arange(r1 - r0), np.arange(r0, r1)] = np.inf
        b = _three_smallest(d)
        with np.errstate(over="ignore"):
            out[r0:r1] = ((b[:, 0] + b[:, 1]) + b[:, 2]) / three
    return out


def knn_f64(xyz):
    """Float64 evaluation of the definition on the float32 positions (P >= 4)."""
    p = np.ascontiguousarray(xyz, dtype=np.float32).astype(np.float64)
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        return knn_ref_numpy(p, np.float64)
    d = cKDTree(p).query(p, k=4)[0][:, 1:]  # the point itself (or a coincident one, also at 0) comes first
    d = d * d
    return ((d[:, 0] + d[:, 1]) + d[:, 2]) / 3.0


def rel_err(a, b64):
    """Largest |a - b| / |b| over the entries with b != 0; entries with b == 0 must be exactly 0 in a."""
    a = np.asarray(a, np.float64)
    zero = b64 == 0
    assert not a[zero].any()
    if zero.all():
        return 0.0
    return float(np.max(np.abs(a[~zero] - b64[~zero]) / np.abs(b64[~zero])))


def _cloud_shell(rng, P):
    """A Gaussian cloud and 10% of the points on a shell at 10x its radius first (create_from_pcd's skybox,
    scene/gaussian_model.py:829-838): the cloud fills about 1/1000 of the bounding box."""
    S = P // 10
    cloud = rng.normal(0.0, 1.0, (P - S, 3))
    mean = cloud.mean(0) if P - S else np.zeros(3)
    radius = np.linalg.norm(cloud.max(0) - mean) if P - S else 1.0
    theta = 2.0 * np.pi * rng.random(S)
    phi = np.arccos(1.0 - 1.4 * rng.random(S))
    shell = radius * 10 * np.stack((np.cos(theta) * np.sin(phi), np.sin(theta) * np.sin(phi), np.cos(phi)), 1) + mean
    return np.concatenate((shell, cloud))


def _plane(rng, P):
    p = rng.random((P, 3)) * 4.0
    p[:, 2] = 0.75
    return p


def _line(rng, P):
    t = rng.random(P)
    return np.stack((3.0 * t - 1.0, 0.5 * t + 2.0, -2.0 * t), 1)


def _identical(rng, P):
    return np.tile(np.array([[0.3, -1.7, 2.9]]), (P, 1))


def _repeat5(rng, P):
    base = rng.random((max(1, P // 5), 3))  # every point at least five times (four coincident others) once P >= 5
    return base[np.arange(P) % len(base)][rng.permutation(P)]


def _lattice(rng, P):
    n = max(1, int(np.ceil(P ** (1.0 / 3.0))))
    g = np.stack(np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij"), -1).reshape(-1, 3)
    return g[rng.permutation(len(g))[:P]].astype(np.float64)


def _centre_cluster(rng, P):
    """Half the points in a tight cluster straddling the centre of the bounding box (neighbours in space, far apart
    in Morton order: the eight octants meet there), the rest uniform in the box, whose corners are pinned."""
    p = rng.random((P, 3)) * 2.0 - 1.0
    p[: P // 2] = rng.normal(0.0, 1e-3, (P // 2, 3))
    if P >= 2:
        p[-1], p[-2] = 1.0, -1.0
    return p


def _two_clusters(rng, P):
    n = P // 8
    return np.concatenate((rng.normal(0.0, 0.1, (n, 3)) + np.array([50.0, -20.0, 5.0]), rng.normal(0.0, 1.0, (P - n, 3))))


SCENES = {
    "cube": lambda rng, P: rng.random((P, 3)),
    "cloud_shell": _cloud_shell,
    "far_offset": lambda rng, P: rng.normal(0.0, 0.05, (P, 3)) + np.array([133.0, -80.0, 40.0]),
    "plane": _plane,
    "line": _line,
    "identical": _identical,
    "repeat5": _repeat5,
    "lattice": _lattice,
    "centre_cluster": _centre_cluster,
    "two_clusters": _two_clusters,
}


def make_scene(name, P, seed=0):
    """(P, 3) float32 positions of the named scene."""
    rng = np.random.default_rng([seed, sorted(SCENES).index(name), P])
    p = np.asarray(SCENES[name](rng, P), dtype=np.float64).reshape(-1, 3)
    assert p.shape == (P, 3)
    return np.ascontiguousarray(p.astype(np.float32))
