"""The scene builders of tests/test_gpu_dispatch.py (helpers.one_tile_scene, helpers.sparse_scene, helpers.equal_depths)
do what those tests rest on, asserted from the oracle alone: a one-tile scene has exactly one non-empty tile with
exactly n entries, and a sparse scene shows a few thousand Gaussians spread over most count blocks of a P-Gaussian
frame.
Every size the GPU tests use is listed here; they import the lists."""
import numpy as np
import pytest

from hlgs_core import synthetic as S
from oracle import oracle as O
from helpers import bin_gauss, equal_depths, one_tile_scene, sparse_scene, tile_counts

# list lengths the GPU tests place on one tile (tests/test_gpu_dispatch.py)
SORT_N = (1024, 1025, 4096, 4097, 8192, 8193, 16384, 16385)  # wave sort | block sort | 1, 2, 3 merge passes
SORT_N_SMALL = (1024, 1025, 4096, 4097)                      # the plain-entry and alt runs
CHUNK_N = (63, 64, 65, 192, 193, 384, 385, 576, 577)         # 64-splat batches; 1, 2, 3 backward chunks, longer ones
CHUNK_N_ALT = (192, 193, 384, 385, 576, 577)
TIE_N = (1025, 4097)
ORDER_N = (600, 2000, 5000)                                  # S, M, L of the frame-order sequence
# Gaussian counts around bin_gauss's switch and k_tile_offsets[_plan]'s code paths: (P, SH degree, bin_gauss, nb)
SPARSE = ((262144, 1, 1024, 256), (262145, 1, 1024, 257), (786432, 1, 1024, 768), (786433, 1, 4096, 193),
          (1048576, 0, 4096, 256), (1048577, 0, 4096, 257), (3145728, 0, 4096, 768), (3145729, 0, 4096, 769))
SPARSE_WH = (320, 200)


def _one_tile(sc, cam, n):
    fr = O.forward(dict(sc), S.cam_numpy(cam), drop_empty=True)
    c = tile_counts(fr)
    assert fr.R == n
    assert (c > 0).sum() == 1 and c.max() == n
    assert c[1 * 4 + 1] == n  # tile (1, 1) of the 4 x 4 grid
    assert np.all(fr.radii == 4)
    return fr


@pytest.mark.parametrize("n,deg", [(n, 0) for n in sorted(set(SORT_N + CHUNK_N))] + [(n, 1) for n in ORDER_N] +
                         [(n, 3) for n in CHUNK_N])
def test_one_tile_scene_fills_exactly_one_tile(n, deg):
    sc, cam = one_tile_scene(n, seed=n, deg=deg)
    assert sc["means3D"].shape == (n, 3) and sc["shs"].shape == (n, (deg + 1) ** 2, 3)
    fr = _one_tile(sc, cam, n)
    if n <= 577:  # some pixel stays live through the whole list: every backward chunk has work
        assert fr.n_contrib.max() == n


@pytest.mark.parametrize("n", sorted(set(SORT_N_SMALL + CHUNK_N_ALT)))
@pytest.mark.parametrize("aa", [True, False])
def test_one_tile_scene_alt(n, aa):
    sc, cam = one_tile_scene(n, seed=n, deg=3 if n in CHUNK_N_ALT else 1, alt=True, aa=aa)
    assert sc["alt"] and sc["dc"].shape == (n, 1, 3)
    fr = _one_tile(sc, cam, n)
    if n <= 577:
        assert fr.n_contrib.max() == n


@pytest.mark.parametrize("n", TIE_N)
def test_equal_depths_keeps_the_tile_and_ties_every_key(n):
    sc, cam = one_tile_scene(n, seed=n)
    fr = _one_tile(equal_depths(sc), cam, n)
    assert np.unique(fr.depths).size == 1
    c = tile_counts(fr)
    t = int(np.argmax(c))
    np.testing.assert_array_equal(fr.point_list[fr.ranges[t, 0]:fr.ranges[t, 1]], np.arange(n, dtype=np.uint32))


@pytest.mark.parametrize("P,deg,bg,nb", SPARSE)
def test_sparse_scene_spreads_over_the_count_blocks(P, deg, bg, nb):
    assert bin_gauss(P) == bg and -(-P // bg) == nb
    W, H = SPARSE_WH
    sc, cam, shown = sparse_scene(P, seed=P % 1000, W=W, H=H, deg=deg)
    assert sc["means3D"].shape == (P, 3)
    fr = O.forward(dict(sc), S.cam_numpy(cam), drop_empty=True)
    vis = np.nonzero(fr.radii > 0)[0]
    assert 0 < vis.size <= shown.size and np.isin(vis, shown).all()  # nothing hidden reaches the frame
    assert np.unique(vis // bg).size > nb // 2
    assert fr.radii[P - 1] > 0 and (P - 1) // bg == nb - 1            # the last count block has an entry
    c = tile_counts(fr)
    assert 0 < c.max() <= 1024 and c.sum() > vis.size                 # short lists; Gaussians span several tiles
