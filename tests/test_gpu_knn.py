"""simple_knn.distCUDA2 on the GPU (csrc/knn.hip) against the all-pairs restatement (tests/knn_ref.py), bit for bit.

The kernel prunes with bounding boxes whose distances round like the point distances, so its output is the all-pairs
result itself, not an approximation: every comparison here is on the float bits.  Where P <= 12,000 the output is also
held to float64 within the bound tests/test_knn_cpu.py derives (1e-6 relative).

Sizes: the small ones (0, 1, 3, 4, 5) and both sides of every size at which a call takes another path
(simple_knn._C.plan gives the side taken, asserted in test_sizes_sit_on_their_thresholds):
- the box of 64 Morton-sorted points, one wave of the search: 63, 64, 65 (one box, one full box, a second box of one);
- the sort tile of 1,024 keys one block of a radix pass histograms and scatters: 1,023, 1,024, 1,025;
- the super-box of 64 boxes = 4,096 points: 4,095, 4,096, 4,097 (one super-box, two);
- the scan over the 256 x tiles digit counts, one block up to 2,048 counts = 8 tiles = 8,192 points, then block totals
  scanned again: 8,192, 8,193.  A third scan level starts above 16,777,216 points (2,048^2 counts), where an all-pairs
  oracle takes hours; it is the same recursive function (scan.hip) one level deeper and is not run here;
- 100,003: many super-boxes, an odd tail, more search blocks than compute units;
- the search's step of 64 super-boxes = 262,144 points, above which a wave tests the super-boxes in more than one step
  and the step's base index is non-zero: 262,144 and 262,145 (64 and 65 super-boxes), on three scenes only because the
  oracle takes over a second there (test_bit_exact_past_one_super_box_step);
- the bounding-box reduction's 256 blocks of 256 points = 65,536, above which its blocks take more than one stride:
  65,536 and 65,537, in the same test.  The bounding box only shapes the Morton keys, so this side changes the order
  the search visits points in and, by the exactness argument, never the result; 100,003 is past it as well.
"""
import functools

import numpy as np
import pytest
import torch

from knn_ref import SCENES, knn_f64, knn_ref, make_scene, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64_BOUND = 1e-6  # tests/test_knn_cpu.py
BIG = 100_003
SIZES = [0, 1, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8192, 8193, BIG]
STEP = 64 * 64 * 64   # points in one step of 64 super-boxes
BBOX = 256 * 256      # points the bounding-box blocks cover in one stride
LARGE = [BBOX, BBOX + 1, STEP, STEP + 1]
LARGE_SCENES = ["centre_cluster", "cloud_shell", "cube"]


@functools.lru_cache(maxsize=None)
def _scene(name, P):
    xyz = make_scene(name, P)
    xyz.setflags(write=False)
    return xyz


@functools.lru_cache(maxsize=None)
def _ref_bits(name, P):
    """The restatement's float bits, computed once per (scene, size) on the GPU and shared."""
    bits = knn_ref(np.array(_scene(name, P)), DEV).cpu().numpy().view(np.uint32)
    bits.setflags(write=False)
    return bits


def _dist(xyz):
    from simple_knn._C import distCUDA2
    out = distCUDA2(torch.from_numpy(np.array(xyz)).to(DEV))
    assert out.dtype == torch.float32 and out.shape == (len(xyz),) and out.device.type == "cuda"
    return out.cpu().numpy()


def test_sizes_sit_on_their_thresholds():
    from simple_knn import _C as K
    assert (K.BOX, K.SUPER, K.SORT_TILE, K.RADIX, K.SCAN_ITEMS) == (64, 64, 1024, 256, 2048)
    assert K.BBOX_BLOCKS == 256
    side = lambda P: tuple(K.plan(P)[k] for k in ("boxes", "super_boxes", "sort_tiles", "scan_levels"))  # noqa: E731
    assert [(K.plan(P)["super_boxes"], K.plan(P)["super_steps"]) for P in (STEP, STEP + 1)] == [(64, 1), (65, 2)]
    assert [K.plan(P)["bbox_strides"] for P in (BBOX, BBOX + 1)] == [1, 2]
    assert K.plan(BIG)["super_steps"] == 1 and K.plan(BIG)["bbox_strides"] == 2
    assert LARGE == [65536, 65537, 262144, 262145]
    assert [side(P)[0] for P in (63, 64, 65)] == [1, 1, 2]              # box
    assert [side(P)[2] for P in (1023, 1024, 1025)] == [1, 1, 2]        # sort tile
    assert [side(P)[1] for P in (4095, 4096, 4097)] == [1, 1, 2]        # super-box
    assert [side(P)[3] for P in (8192, 8193)] == [1, 2]                 # scan: one block, block totals scanned again
    assert side(BIG) == (1563, 25, 98, 2)
    assert all(P in SIZES for P in (63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8192, 8193))


@pytest.mark.parametrize("P", SIZES)
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_bit_exact_against_restatement(scene, P):
    xyz = _scene(scene, P)
    got = _dist(xyz)
    want = _ref_bits(scene, P)
    bad = np.flatnonzero(got.view(np.uint32) != want)
    assert bad.size == 0, (f"{bad.size} of {P} differ, first at {bad[:5]}: got {got[bad[:5]]}, "
                           f"want {want.view(np.float32)[bad[:5]]}")
    if P <= 3:
        assert np.isposinf(got).all()
    elif P <= 12000:
        err = rel_err(got, knn_f64(xyz))
        print(f"{scene} P={P}: rel err to float64 {err:.3g}")
        assert err <= F64_BOUND
    if scene in ("identical", "repeat5") and P >= 5:
        assert not got.any()


@pytest.mark.parametrize("P", LARGE)
@pytest.mark.parametrize("scene", LARGE_SCENES)
def test_bit_exact_past_one_super_box_step(scene, P):
    """Both sides of the 64-super-box step of the search and of the bounding-box reduction's stride."""
    got = _dist(_scene(scene, P))
    want = _ref_bits(scene, P)
    bad = np.flatnonzero(got.view(np.uint32) != want)
    assert bad.size == 0, (f"{bad.size} of {P} differ, first at {bad[:5]}: got {got[bad[:5]]}, "
                           f"want {want.view(np.float32)[bad[:5]]}")


@pytest.mark.parametrize("P", [1, 2, 3])
def test_fewer_than_three_neighbours_give_inf(P):
    got = _dist(_scene("cube", P))
    assert got.shape == (P,) and np.isposinf(got).all()


def test_no_points():
    from simple_knn._C import distCUDA2
    out = distCUDA2(torch.empty((0, 3), device=DEV))
    assert out.shape == (0,) and out.dtype == torch.float32 and out.device.type == "cuda"


def test_two_runs_are_bitwise_equal():
    xyz = _scene("cloud_shell", BIG)
    a, b = _dist(xyz), _dist(xyz)
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    np.testing.assert_array_equal(a.view(np.uint32), _ref_bits("cloud_shell", BIG))


def test_side_stream_equals_default_stream():
    """The call runs on torch's current stream: its input is uploaded on a side stream behind a long kernel, so
    kernels launched on any other stream would read the buffer before the upload."""
    from simple_knn._C import distCUDA2
    xyz = _scene("two_clusters", 8193)
    want = _dist(xyz)
    host = torch.from_numpy(np.array(xyz)).pin_memory()
    side = torch.cuda.Stream()
    big = torch.randn(4096, 4096, device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(8):
            big = big @ big * 1e-3
        dev = torch.zeros((len(xyz), 3), device=DEV)
        dev.copy_(host, non_blocking=True)
        out = distCUDA2(dev)
    side.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32))
    torch.cuda.synchronize()


def test_non_contiguous_and_float64_inputs():
    from simple_knn._C import distCUDA2
    xyz = _scene("cube", 4097)
    want = _ref_bits("cube", 4097)
    t = torch.from_numpy(np.ascontiguousarray(xyz.T)).to(DEV).T  # (3, P).T: strides (1, P)
    assert t.shape == (4097, 3) and not t.is_contiguous()
    np.testing.assert_array_equal(distCUDA2(t).cpu().numpy().view(np.uint32), want)
    d = torch.from_numpy(xyz.astype(np.float64)).to(DEV)         # float64 values that are exactly the float32 ones
    out = distCUDA2(d)
    assert out.dtype == torch.float32
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), want)


def test_initial_log_scales():
    """scene/gaussian_model.py:848-852 on the device: finite on coincident points (the clamp), and the reference's
    expression applied to the restatement's distances."""
    from hlgs_core import scene
    xyz = torch.from_numpy(np.array(_scene("repeat5", 4095))).to(DEV)
    got = scene.initial_log_scales(xyz)
    assert got.shape == (4095, 3) and bool(torch.isfinite(got).all())
    assert bool((got == torch.log(torch.sqrt(torch.tensor(1e-7, device=DEV)))).all())

    S = 409
    sky = torch.from_numpy(np.array(_scene("cloud_shell", 4095))).to(DEV)
    ref = torch.from_numpy(_ref_bits("cloud_shell", 4095).view(np.float32).copy()).to(DEV)
    for skybox_points, scaffold in ((S, False), (0, False), (S, True)):
        dist2 = torch.clamp_min(ref.clone(), 0.0000001)
        if not scaffold and skybox_points > 0:
            dist2[:skybox_points] *= 10
            dist2[skybox_points:] = torch.clamp_max(dist2[skybox_points:], 10)
        want = torch.log(torch.sqrt(dist2))[..., None].repeat(1, 3)
        got = scene.initial_log_scales(sky, skybox_points=skybox_points, scaffold=scaffold)
        assert torch.equal(got, want)
