"""The n-ary mode of the SPT path on the GPU (csrc/spt_build.hip, csrc/stream.hip, hlgs_core.spt, SPTCache) against the
host build and the numpy restatement of the contract (tests/spt_nary_ref.py), on merged scene hierarchies
(tests/hier_merge_ref.py and merge_dynamic_hierarchies itself).  The host build of every case is checked against the
restatement on the CPU (tests/test_spt_nary_cpu.py); CPU references are computed once and shared."""
import numpy as np
import pytest
import torch

import spt_nary_cases as C
import spt_nary_ref as NR
from hlgs_core import hierarchy as H
from hlgs_core import mcmc, spt
from hlgs_core import synthetic as S
from oracle import oracle as O
from oracle import spt_ref as SR

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = ("xyz", "f_dc", "opacity", "scaling", "rotation", "f_rest")
SHAPES = {"xyz": (3,), "f_dc": (1, 3), "opacity": (1,), "scaling": (3,), "rotation": (4,), "f_rest": (15, 3)}

_host = {}


def _host_build(name, sky, volume, min_size):
    """The n-ary host build of a case, integers checked against the restatement."""
    key = (name, sky, volume, min_size)
    if key not in _host:
        nodes, xyz, scaling = C.tensors(name, sky)
        got = C.to_numpy(spt.build_hierarchical_spt(nodes, xyz, scaling, sky, volume, C.TG, min_size, nary=True))
        want = C.reference(*key)
        for k in C.INTS:
            np.testing.assert_array_equal(got[k], want[k], err_msg=f"host build against restatement: {k}")
        _host[key] = got
    return _host[key]


def _packed_views(xyz, scaling):
    """xyz and scaling as SPTCache lays them out: strided views of one packed pinned host table."""
    w = [int(np.prod(SHAPES[k])) for k in NAMES] * 3
    hw = -(-sum(w) // 16) * 16
    host = torch.zeros((xyz.shape[0], hw), dtype=torch.float32, pin_memory=True)
    off = {k: sum(w[:i]) for i, k in enumerate(NAMES)}
    vx, vs = host[:, off["xyz"]:off["xyz"] + 3], host[:, off["scaling"]:off["scaling"] + 3]
    vx.copy_(xyz)
    vs.copy_(scaling)
    assert not vx.is_contiguous() and vx.is_pinned()
    return vx, vs


def _device(nodes, xyz, scaling, root, volume, min_size, tg=C.TG, **kw):
    t = lambda a: torch.as_tensor(a).to(DEV)  # noqa: E731
    return spt.build_hierarchical_spt_device(t(nodes), t(xyz), t(scaling), root, volume, tg, min_size, **kw)


# ------------------------------------------------------------------------------------------------ device against host
@pytest.mark.parametrize("layout", ["device", "packed_pinned_views"])
@pytest.mark.parametrize("spheres", [True, False])
@pytest.mark.parametrize("name,sky,volume,min_size", C.CASES)
def test_device_build_matches_host_build(name, sky, volume, min_size, spheres, layout):
    nodes, xyz, scaling = C.tensors(name, sky)
    want = _host_build(name, sky, volume, min_size)
    if layout == "device":
        args = (nodes.to(DEV), xyz.to(DEV), scaling.to(DEV))
    else:
        args = (nodes,) + _packed_views(xyz, scaling)
    got = spt.build_hierarchical_spt_device(*args, sky, volume, C.TG, min_size, use_bounding_spheres=spheres, nary=True)
    assert got.pop("nary") is True and set(got) == set(spt.SPT_KEYS)
    assert all(v is None or (v.is_cuda and v.is_contiguous()) for v in got.values())
    C.compare(got, want, spheres)


def test_one_spt_larger_than_a_workgroup():
    want = _host_build(*C.BIG_SPT_CASE)
    assert np.diff(want["SPT_starts"]).max() > 1024
    C.compare(_device(*C.scene("k8"), 0, C.BIG_SPT_CASE[2], C.BIG_SPT_CASE[3], nary=True), want)


# ------------------------------------------------------------------------------------------------ GPU to GPU
def test_merger_output_goes_straight_into_the_build():
    chunks, centers = C.chunks_of("k3")
    out = H.merge_dynamic_hierarchies([tuple(torch.tensor(a, device=DEV) for a in ch) for ch in chunks], centers)
    pos, ls, nodes = out[0], out[3], out[5]
    got = spt.build_hierarchical_spt_device(nodes, pos, ls, 0, 2.5e-5, C.TG, 10, nary=True)
    want = NR.build_spt_nary(nodes.cpu().numpy(), pos.cpu().numpy(), ls.cpu().numpy(), 0, 2.5e-5, C.TG, 10)
    assert len(want["SPT_root_hierarchy_indices"]) >= 4 and (nodes[:, 2] == 1).sum() >= 20
    got.pop("nary")
    C.compare(got, want)


# ------------------------------------------------------------------------------------------------ extreme trees
def _rows(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, 3, generator=g) * 3, torch.randn(n, 3, generator=g) * 0.3 - 2


def _star(n):
    nd = np.zeros((n + 1, 6), np.int32)
    nd[0] = (0, -1, n, 1, 0, 0)
    for i in range(1, n + 1):
        nd[i] = (1, 0, 0, i + 1, i + 1 if i < n else 0, 0)
    return nd


def _chain(depth):
    nd = np.zeros((depth + 1, 6), np.int32)
    for i in range(depth + 1):
        nd[i] = (i, i - 1, 1 if i < depth else 0, i + 1, 0, 0)
    return nd


@pytest.mark.parametrize("volume", [0.0, 1e30])
def test_star_root_with_300_children(volume):
    """volume 0: the root expands in the upper walk; 1e30: the root is the one SPT.  Either way the 300 children are
    one level: one read-back after the validation, one per level of a walk (two levels, the second expands nothing),
    one for the candidates, one for the sizes."""
    nodes = torch.tensor(_star(300))
    xyz, scaling = _rows(301, 1)
    want = C.to_numpy(spt.build_hierarchical_spt(nodes, xyz, scaling, 0, volume, C.TG, 10, nary=True))
    ref = NR.build_spt_nary(nodes.numpy(), xyz.numpy(), scaling.numpy(), 0, volume, C.TG, 10)
    for k in C.INTS:
        np.testing.assert_array_equal(want[k], ref[k], err_msg=k)
    got = _device(nodes, xyz, scaling, 0, volume, 10, nary=True)
    assert spt.last_device_build["host_syncs"] <= 8
    C.compare(got, want)
    assert len(want["SPT_root_hierarchy_indices"]) == (1 if volume else 0)


@pytest.mark.parametrize("volume", [0.0, 1e30])
def test_chain_of_299_one_child_nodes(volume):
    nodes = torch.tensor(_chain(299))
    xyz, scaling = _rows(300, 2)
    want = C.to_numpy(spt.build_hierarchical_spt(nodes, xyz, scaling, 0, volume, C.TG, 10, nary=True))
    ref = NR.build_spt_nary(nodes.numpy(), xyz.numpy(), scaling.numpy(), 0, volume, C.TG, 10)
    for k in C.INTS:
        np.testing.assert_array_equal(want[k], ref[k], err_msg=k)
    got = _device(nodes, xyz, scaling, 0, volume, 10, nary=True)
    C.compare(got, want)
    assert want["upper_tree_nodes"].shape[0] == (1 if volume else 300)


# ------------------------------------------------------------------------------------------------ binary equivalence
_binary = {}


def _binary_hierarchy(n, sky):
    if (n, sky) not in _binary:
        h = S.make_dynamic_hierarchy(S.make_gaussians(n, 0, S.make_camera(256, 192), seed=n), skybox_points=sky,
                                     seed=n)
        nodes = torch.tensor(h["nodes"])
        nodes[:, 3] = torch.where(nodes[:, 2] == 2, nodes[:, 3], torch.zeros_like(nodes[:, 3]))
        _binary[(n, sky)] = (nodes, torch.tensor(h["means3D"]), torch.log(torch.tensor(h["scales"])))
    return _binary[(n, sky)]


@pytest.mark.parametrize("n,sky,volume,min_size", [(3000, 5, 5.0, 20), (6000, 0, 2.0, 50), (2000, 3, 20.0, 10)])
def test_nary_mode_equals_binary_mode_on_the_device(n, sky, volume, min_size):
    nodes, xyz, scaling = _binary_hierarchy(n, sky)
    a = _device(nodes, xyz, scaling, sky, volume, min_size)
    b = _device(nodes, xyz, scaling, sky, volume, min_size, nary=True)
    assert set(a) == set(spt.SPT_KEYS) and b.pop("nary") is True
    assert a["SPT_root_hierarchy_indices"].numel() > 3
    for k in spt.SPT_KEYS:
        assert torch.equal(a[k], b[k]), k
    # and the cuts of the binary upper tree, level walk and flat
    cam = _ring_cameras(np.asarray(xyz.mean(0)), 2.0)[0]
    planes = spt.extract_frustum_planes(cam["projmatrix"])
    oa, ob = spt.upper_tree_order(a["upper_tree_nodes"]), spt.upper_tree_order(a["upper_tree_nodes"], nary=True)
    assert oa is not None and torch.equal(oa, ob)
    args = (a["upper_tree_nodes"], a["upper_tree_xyz"], a["bounding_sphere_radii"], a["min_distance_squared"], planes,
            cam["campos"], 0.05)
    want = spt.upper_tree_cut(*args)
    assert want.numel() > 8
    assert torch.equal(spt.upper_tree_cut(*args, nary=True), want)
    assert torch.equal(spt.upper_tree_cut(*args, order=ob, nary=True), want)


# ------------------------------------------------------------------------------------------------ cuts
def _ring_cameras(centre, radius, n=6, W=320, Hh=240):
    """n cameras on a ring around `centre` in the x-z plane (radius: one distance or one per camera), each looking at
    the centre."""
    cams = []
    radii = list(radius) if np.ndim(radius) else [radius] * n
    n = len(radii)
    for k, radius in enumerate(radii):
        a = 2 * np.pi * k / n
        pos = np.asarray(centre, np.float64) + radius * np.array([np.cos(a), 0.15 * (k % 3 - 1), np.sin(a)])
        z = np.asarray(centre, np.float64) - pos
        z /= np.linalg.norm(z)
        x = np.cross([0.0, 1.0, 0.0], z)
        x /= np.linalg.norm(x)
        y = np.cross(z, x)
        R = np.stack([x, y, z], axis=1)  # camera-to-world
        cams.append(S.make_camera(W, Hh, R=R, T=-R.T @ pos))
    return cams


_cut = {}


def _cut_scene():
    """The whole K = 8 scene as an upper tree (volume 0: every inner node expands, no SPT), on the device, with the six
    ring cameras and the restatement's cut of each view and of the two unions."""
    if not _cut:
        b = _host_build("k8", 0, 0.0, 10)
        assert b["upper_tree_nodes"].shape[0] == C.scene("k8")[0].shape[0] and len(b["SPT_starts"]) == 1
        cams = _ring_cameras([2.0, 2.0, 2.0], C.CUT_RADII)
        views = C.CUT_VIEWS
        refs = []
        for v, dmul in views:
            planes = np.stack([spt.extract_frustum_planes(cams[k]["projmatrix"]).numpy() for k in v])
            campos = np.stack([cams[k]["campos"].numpy().reshape(-1)[:3] for k in v])
            refs.append(NR.upper_tree_cut_nary(b["upper_tree_nodes"], b["upper_tree_xyz"], b["bounding_sphere_radii"],
                                               b["min_distance_squared"], planes, campos, dmul))
        dev = {k: torch.tensor(b[k], device=DEV) for k in ("upper_tree_nodes", "upper_tree_xyz",
                                                           "bounding_sphere_radii", "min_distance_squared")}
        _cut.update(b=b, cams=cams, views=views, refs=refs, dev=dev)
    return _cut


def test_cut_scene_takes_every_path_of_the_level_walk():
    """From the restatement alone: the n-ary level walk runs every level in one workgroup of 1,024 threads, so the
    sizes asked for are a level in (1,024, 2,048] entries (two entries per thread) and one above 2,048 (three and more
    per thread, several batches of the rank loop's runs); and each of the four node states on at least 5 % of some
    view's visited nodes."""
    s = _cut_scene()
    sizes = [n for _, _, lv in s["refs"] for n in lv]
    assert any(1024 < n <= 2048 for n in sizes) and any(n > 2048 for n in sizes)
    for state in range(4):
        assert max(np.mean([st == state for st in states.values()]) for _, states, _ in s["refs"][:6]) >= 0.05, state


@pytest.mark.parametrize("flat", [False, True])
@pytest.mark.parametrize("view", range(8))
def test_cuts_match_the_restatement(view, flat):
    s = _cut_scene()
    d, cams, (v, dmul) = s["dev"], s["cams"], s["views"][view]
    planes = torch.stack([spt.extract_frustum_planes(cams[k]["projmatrix"]) for k in v])
    campos = torch.stack([cams[k]["campos"].reshape(-1)[:3] for k in v])
    order = None
    if flat:
        order = spt.upper_tree_order(d["upper_tree_nodes"], nary=True)
        assert order is not None
    got = spt.upper_tree_cut(d["upper_tree_nodes"], d["upper_tree_xyz"], d["bounding_sphere_radii"],
                             d["min_distance_squared"], planes, campos, dmul, order=order, nary=True)
    want = s["refs"][view][0]
    assert len(want) > 100
    np.testing.assert_array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("tree,flat", [("star", False), ("star", True), ("chain", False)])
def test_extreme_trees_through_the_cuts(tree, flat):
    """The 300-child star (one level whose rank loop runs 300 rounds) and the chain of 299 one-child nodes (300 levels
    of one entry) as upper trees: every inner node expands (a tiny distance multiplier), so the walk reaches the
    last rank and the last level.  The chain is deeper than the flat cut's 64 levels: the order builder refuses it."""
    nodes = torch.tensor(_star(300) if tree == "star" else _chain(299))
    xyz, scaling = _rows(nodes.shape[0], 3)
    b = spt.build_hierarchical_spt(nodes, xyz, scaling, 0, 0.0, C.TG, 10, nary=True)
    assert b["upper_tree_nodes"].shape[0] == nodes.shape[0]
    cam = torch.tensor([0.5, -0.25, 1.0])
    want, states, sizes = NR.upper_tree_cut_nary(b["upper_tree_nodes"].numpy(), b["upper_tree_xyz"].numpy(), None,
                                                 b["min_distance_squared"].numpy(), None, cam.numpy(), 1e-9,
                                                 use_frustum=False)
    assert sizes == ([1, 300] if tree == "star" else [1] * 300) and len(want) == (300 if tree == "star" else 1)
    d = {k: b[k].to(DEV) for k in ("upper_tree_nodes", "upper_tree_xyz", "bounding_sphere_radii",
                                   "min_distance_squared")}
    order = spt.upper_tree_order(d["upper_tree_nodes"], nary=True)
    assert (order is None) == (tree == "chain")
    got = spt.upper_tree_cut(d["upper_tree_nodes"], d["upper_tree_xyz"], d["bounding_sphere_radii"],
                             d["min_distance_squared"], None, cam, 1e-9, use_frustum=False,
                             order=order if flat else None, nary=True)
    np.testing.assert_array_equal(got.cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------ cache
class _Oracle:
    """The cache run on the CPU: the restatement's n-ary coarse cut fed to oracle.spt_ref.cache_pass."""

    def __init__(self, b, storage, opt, sky, rtol):
        self.b, self.sky, self.rtol = b, sky, rtol
        tens = [storage[k].numpy().copy() for k in NAMES]
        zero = [np.zeros_like(t) for t in tens]
        self.host = tens + ([opt[k]["exp_avgs"].numpy().copy() for k in NAMES] if opt else zero) + \
            ([opt[k]["exp_avgs_sqs"].numpy().copy() for k in NAMES] if opt else [z.copy() for z in zero])
        # the skybox rows are loaded with zero moments (train_post.py:208-231); there are none here
        self.dev = [h[:sky].copy() for h in self.host]
        self.render, self.n_loaded = np.arange(sky, dtype=np.int32), 0
        self.prev = (np.zeros(0, np.int32), np.zeros(0, np.float32), np.zeros(0, np.int32))

    def step(self, cam):
        b = self.b
        planes = spt.extract_frustum_planes(cam["projmatrix"]).numpy()[None]
        campos = cam["campos"].numpy().reshape(1, -1)[:, :3]
        cut_fn = lambda i, d: O.spt_cut(b["SPT_gaussian_indices"], b["SPT_starts"], b["SPT_max"],  # noqa: E731
                                        b["SPT_min"], i, d, compat=True)
        coarse = NR.upper_tree_cut_nary(b["upper_tree_nodes"], b["upper_tree_xyz"], b["bounding_sphere_radii"],
                                        b["min_distance_squared"], planes, campos, 1.0)[0]
        r = SR.cache_pass(b["upper_tree_nodes"], b["upper_tree_xyz"], coarse, campos, 1.0, *self.prev, self.render,
                          self.n_loaded, self.sky, self.rtol, 0.05, cut_fn)
        keep, wb, lfd = r["keep_mask"], r["write_back_indices"], r["load_from_disk_indices"]
        for k in range(len(self.host)):
            self.host[k][wb] = self.dev[k][~keep]
            self.dev[k] = np.concatenate([self.dev[k][keep], self.host[k][lfd]])
        self.prev = (r["SPT_indices"], r["SPT_distances"], r["SPT_counts"])
        self.render, self.n_loaded = r["render_indices"], len(lfd)
        r["coarse"] = coarse
        return r


def _dev_list(c):
    return [c.params[k] for k in NAMES] + [c.exp_avgs[k] for k in NAMES] + [c.exp_avg_sqs[k] for k in NAMES]


def _storage(G, seed, moments):
    rng = np.random.default_rng(seed)
    storage = {k: torch.tensor(rng.normal(size=(G,) + SHAPES[k]).astype(np.float32)) for k in NAMES}
    opt = None
    if moments:
        opt = {k: {"exp_avgs": torch.tensor(rng.normal(size=(G,) + SHAPES[k]).astype(np.float32)),
                   "exp_avgs_sqs": torch.tensor(rng.random(size=(G,) + SHAPES[k]).astype(np.float32))} for k in NAMES}
    return storage, opt


@pytest.mark.parametrize("moments", [False, True])
@pytest.mark.parametrize("flat", [True, False])
def test_cache_over_a_merged_scene_matches_the_restatement(flat, moments):
    from hlgs_core.spt_cache import SPTCache
    b = _host_build(*C.CASES[0])
    G = C.scene("k3")[0].shape[0]
    storage, opt = _storage(G, 5, moments)
    spt_dict = {k: (torch.tensor(v) if v is not None else None) for k, v in b.items()}
    spt_dict["nary"] = True
    cache = SPTCache(storage, spt_dict, 0, opt_storage=opt, reuse_tolerance=0.9, flat_cut=flat)
    assert cache.nary and (cache.cut_order is not None) == flat
    orc = _Oracle(b, storage, opt, 0, 0.9)
    cams = _ring_cameras([1.5, 1.5, 0.0], 1.0, n=7)
    cams.append(cams[0])
    reused = loaded = 0
    for step, cam in enumerate(cams):
        got = cache.step(cam["projmatrix"], cam["campos"])
        want = orc.step(cam)
        pl = cache.last_plan
        n = int(cache._cut_count[0])
        np.testing.assert_array_equal(cache._cut[:n].cpu().numpy(), want["coarse"], err_msg=f"coarse cut view {step}")
        for k in ("SPT_indices", "SPT_distances", "SPT_counts", "load_from_disk_indices"):
            np.testing.assert_array_equal(pl[k].cpu().numpy(), want[k], err_msg=f"{k} view {step}")
        np.testing.assert_array_equal(got.cpu().numpy(), want["render_indices"])
        np.testing.assert_array_equal(pl["write_back_indices"].cpu().numpy(), want["write_back_indices"])
        for t, (g, w) in enumerate(zip(_dev_list(cache), orc.dev)):
            np.testing.assert_array_equal(g.detach().cpu().numpy(), w, err_msg=f"tensor {t} view {step}")
        reused += want["n_kept"]
        loaded += len(want["load_SPT_indices"])
        with torch.no_grad():  # training changes the resident rows between views
            for t, g in enumerate(_dev_list(cache)):
                g.add_(0.001 * (step + 1) * (t + 1))
        for t in range(len(orc.dev)):
            orc.dev[t] = (orc.dev[t] + np.float32(0.001 * (step + 1) * (t + 1))).astype(np.float32)
    assert reused > 0 and loaded > 3
    cache.sync_storage()
    host = [cache.storage[k] for k in NAMES] + [cache.opt_storage[k]["exp_avgs"] for k in NAMES] + \
           [cache.opt_storage[k]["exp_avgs_sqs"] for k in NAMES]
    for t, (h, w) in enumerate(zip(host, orc.host)):
        np.testing.assert_array_equal(h.numpy(), w, err_msg=f"host tensor {t}")


def test_densify_round_refuses_an_nary_cache():
    from hlgs_core.spt_cache import SPTCache
    b = _host_build(*C.CASES[0])
    nodes = C.tensors("k3")[0]
    G = nodes.shape[0]
    storage, _ = _storage(G, 6, False)
    spt_dict = {k: (torch.tensor(v) if v is not None else None) for k, v in b.items()}
    spt_dict["nary"] = True
    cache = SPTCache(storage, spt_dict, 0)
    cam = _ring_cameras([1.5, 1.5, 0.0], 1.0, n=7)[0]
    cache.step(cam["projmatrix"], cam["campos"])
    cache.sync_storage()
    before, resident = cache.host.clone(), cache.render_indices.clone()
    with pytest.raises(ValueError, match="binary"):
        mcmc.densify_round(cache, nodes, G, cap_max=G, seed=1, spt_args=dict(SPT_Root_Volume=2.5e-5,
                                                                              target_granularity=C.TG))
    torch.cuda.synchronize()
    assert torch.equal(cache.host, before) and torch.equal(cache.render_indices, resident)


# ------------------------------------------------------------------------------------------------ malformed tables
@pytest.mark.parametrize("name", sorted(C.malformed()))
def test_malformed_table_is_rejected_and_the_next_build_is_right(name):
    _, xyz, scaling = C.hand()
    a = C.HAND_ARGS
    with pytest.raises(RuntimeError):
        _device(C.malformed()[name], xyz, scaling, a["root"], a["volume"], a["min_size"], tg=a["tg"], nary=True)
    got = _device(C.HAND_NODES, xyz, scaling, a["root"], a["volume"], a["min_size"], tg=a["tg"], nary=True)
    got.pop("nary")
    C.compare(got, NR.build_spt_nary(*C.hand(), **a))


def test_default_mode_on_the_device_still_rejects_a_one_child_node():
    nodes, xyz, scaling = C.hand()
    nodes[12, 3] = 0  # (the binary validation range-checks every first_child, a leaf's too)
    a = C.HAND_ARGS
    with pytest.raises(RuntimeError, match="binary hierarchy"):
        _device(nodes, xyz, scaling, a["root"], a["volume"], a["min_size"], tg=a["tg"])
