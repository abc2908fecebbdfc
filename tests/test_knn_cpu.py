"""simple_knn.distCUDA2 without a GPU: the restatement the GPU tests compare against (tests/knn_ref.py) is itself
checked against float64 and against a second implementation, and the package surface (import path, argument
errors, exported symbols and their ctypes signatures, hlgs_core.scene.initial_log_scales) is checked.

Float64 bound: each value is a sum of three squared distances, every one three subtractions, three squarings and two
additions of non-negative terms, then two additions and a division: along any path at most about eight float32
roundings of relative size 2^-24 = 6e-8, so at most 5e-7 relative; the bound asserted is 1e-6.  A neighbour swapped
between the float32 and the float64 ranking changes nothing: the swapped distances differ by less than their rounding.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from hlgs_core import _lib as L
from knn_ref import SCENES, knn_f64, knn_ref, knn_ref_numpy, make_scene, rel_err

F64_BOUND = 1e-6


@pytest.mark.parametrize("P", [4, 65, 12000])
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_restatement_matches_float64(scene, P):
    xyz = make_scene(scene, P)
    got = knn_ref(xyz).numpy()
    assert got.dtype == np.float32 and got.shape == (P,)
    err = rel_err(got, knn_f64(xyz))
    print(f"{scene} P={P}: rel err {err:.3g}")
    assert err <= F64_BOUND


@pytest.mark.parametrize("scene", sorted(SCENES))
def test_torch_and_numpy_restatements_agree_bitwise(scene):
    xyz = make_scene(scene, 2000)
    a, b = knn_ref(xyz).numpy(), knn_ref_numpy(xyz)
    assert a.dtype == b.dtype == np.float32
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("P", [0, 1, 2, 3])
def test_restatement_with_fewer_than_three_neighbours(P):
    got = knn_ref(make_scene("cube", P))
    assert got.shape == (P,) and bool(torch.isinf(got).all()) and bool((got > 0).all())


def test_scene_properties():
    """The scenes are what the GPU tests take them for."""
    assert not knn_ref(make_scene("identical", 500)).any()
    assert not knn_ref(make_scene("repeat5", 500)).any()       # every point has four coincident others
    assert not knn_ref(make_scene("repeat5", 503)).any()       # also when 5 does not divide P
    lat = knn_ref(make_scene("lattice", 1000)).numpy()           # the full 10^3 lattice: three unit neighbours each
    np.testing.assert_array_equal(lat, np.ones(1000, np.float32))
    p = make_scene("plane", 300)
    assert np.ptp(p[:, 2]) == 0 and np.ptp(p[:, 0]) > 0
    sky = make_scene("cloud_shell", 12000)
    ext = sky.max(0) - sky.min(0)
    cloud = sky[1200:]
    assert np.prod((cloud.max(0) - cloud.min(0)) / ext) < 2e-3  # the cloud fills ~1/1000 of the bounding box
    c = make_scene("centre_cluster", 4096)
    mid = (c.max(0) + c.min(0)) / 2
    near = np.abs(c - mid).max(1) < 0.01
    assert near.sum() >= 2048 and len({tuple(r) for r in (c[near] > mid)}) == 8  # all eight octants at the centre


def test_import_path():
    import simple_knn
    import simple_knn._C
    from simple_knn._C import distCUDA2
    assert simple_knn.distCUDA2 is distCUDA2 and callable(distCUDA2)


def test_argument_errors():
    from simple_knn._C import distCUDA2
    with pytest.raises(RuntimeError, match=r"\(num_points, 3\)"):
        distCUDA2(torch.zeros(7, 2))
    with pytest.raises(RuntimeError, match=r"\(num_points, 3\)"):
        distCUDA2(torch.zeros(9))
    with pytest.raises(RuntimeError, match="HIP device|device tensors"):  # no CPU path, with or without a GPU present
        distCUDA2(torch.zeros(7, 3))


def test_exports_and_signatures():
    lib = L.load()
    assert {"hlgs_knn_scratch_size", "hlgs_knn_mean_dist2"} <= set(L.header_functions())
    assert lib.hlgs_knn_scratch_size.restype is C.c_size_t and lib.hlgs_knn_scratch_size.argtypes == [C.c_int]
    assert lib.hlgs_knn_mean_dist2.restype is C.c_int
    assert lib.hlgs_knn_mean_dist2.argtypes == [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]


def test_scratch_size_and_c_argument_errors():
    lib = L.load()
    sizes = [lib.hlgs_knn_scratch_size(P) for P in (0, 1, 1000, 1_000_000)]
    assert sizes == sorted(sizes) and all(s % 256 == 0 for s in sizes)
    # two (key, index) buffer pairs and the sorted float4 rows
    assert sizes[3] >= 1_000_000 * (4 * 4 + 16)
    assert lib.hlgs_knn_mean_dist2(-1, None, None, None, None) == 1  # HLGS_ERR_ARG
    assert lib.hlgs_last_error() == b"P < 0"
    assert lib.hlgs_knn_mean_dist2(5, None, None, None, None) == 1
    assert lib.hlgs_last_error() == b"missing tensor"
    assert lib.hlgs_knn_mean_dist2(0, None, None, None, None) == 0   # P == 0 launches nothing


def test_plan_constants_match_header():
    from simple_knn import _C as K
    txt = open(L.HEADER).read()
    macro = lambda n: int(re.search(rf"#define {n} (\d+)", txt).group(1))  # noqa: E731
    assert (K.BOX, K.SUPER, K.SORT_TILE) == (macro("HLGS_KNN_BOX"), macro("HLGS_KNN_SUPER"),
                                             macro("HLGS_KNN_SORT_TILE"))
    # the constants plan() mirrors from the sources that have no header macro
    csrc = os.path.join(L.PKG_DIR, "csrc")
    const = lambda f, n: int(re.search(rf"constexpr int {n} = (\d+);", open(os.path.join(csrc, f)).read()).group(1))  # noqa: E731
    assert K.RADIX == 1 << const("knn.hip", "kRadixBits")
    assert K.SCAN_ITEMS == const("hlgs_internal.h", "kScanItems")
    assert K.BBOX_BLOCKS == const("knn.hip", "kBoxParts")
    assert K.plan(0) == dict(boxes=0, super_boxes=0, super_steps=0, sort_tiles=0, scan_levels=0, bbox_strides=0)
    assert K.plan(64)["boxes"] == 1 and K.plan(65)["boxes"] == 2
    assert K.plan(4096)["super_boxes"] == 1 and K.plan(4097)["super_boxes"] == 2
    assert K.plan(1024)["sort_tiles"] == 1 and K.plan(1025)["sort_tiles"] == 2
    assert K.plan(8192)["scan_levels"] == 1 and K.plan(8193)["scan_levels"] == 2
    assert K.plan(262144)["super_steps"] == 1 and K.plan(262145)["super_steps"] == 2
    assert K.plan(65536)["bbox_strides"] == 1 and K.plan(65537)["bbox_strides"] == 2


def test_initial_log_scales_matches_reference_expression(monkeypatch):
    """hlgs_core.scene.initial_log_scales against the torch expression of scene/gaussian_model.py:848-852 applied to
    the restatement's distances (distCUDA2 itself needs a GPU: the restatement stands in for it here)."""
    from hlgs_core import scene
    from simple_knn import _C as K
    monkeypatch.setattr(K, "distCUDA2", lambda xyz: knn_ref(xyz))
    S = 300
    xyz = torch.from_numpy(make_scene("cloud_shell", 3000))
    xyz[S:S + 50] = xyz[S]  # coincident points: distance 0 before the clamp

    def expected(skybox_points, scaffold_file):
        dist2 = torch.clamp_min(knn_ref(xyz), 0.0000001)
        if scaffold_file == "" and skybox_points > 0:
            dist2[:skybox_points] *= 10
            dist2[skybox_points:] = torch.clamp_max(dist2[skybox_points:], 10)
        return torch.log(torch.sqrt(dist2))[..., None].repeat(1, 3)

    for sky, scaffold in ((S, False), (0, False), (S, True)):
        got = scene.initial_log_scales(xyz, skybox_points=sky, scaffold=scaffold)
        want = expected(sky, "scaffold.ply" if scaffold else "")
        assert got.shape == (3000, 3) and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
        assert torch.equal(got, want)
    assert scene.initial_log_scales(xyz, S)[S, 0] == torch.log(torch.sqrt(torch.tensor(1e-7)))
    assert not torch.equal(scene.initial_log_scales(xyz, S), scene.initial_log_scales(xyz, 0))
