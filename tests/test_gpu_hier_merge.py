"""The chunk merger on the GPU (csrc/hier_merge.hip, hlgs_core.hierarchy.merge_dynamic_hierarchies) against the
recursive numpy restatement of tests/hier_merge_ref.py.

Bit-exact, everything: the node table (all six columns), chunk_roots and every float row (pos, SH, alpha, log-scales,
rot).  The operation is copies, one multiply and a fixed-order float32 formula on both sides, so there is no tolerance."""
import functools

import numpy as np
import pytest
import torch

import hier_merge_ref as R
from hlgs_core import hierarchy as H

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLOATS = ("pos", "shs", "alpha", "log_scales", "rot")

# leaves per chunk: below, at and above a wave, the first sizes with more than one workgroup per launch (1,000 leaves
# are 1,999 rows), and a large one.  The kernels have no fused small-subtree path, so there is no cap to bracket.
CASES = [("uniform", n, 2, 3, False) for n in (1, 2, 3, 63, 64, 65, 1000)] + [
    ("uniform", 20011, 2, 48, False),
    ("uniform", 1000, 1, 12, False), ("uniform", 1000, 3, 48, False), ("uniform", 1000, 8, 3, False),
    ("uniform", 65, 3, 12, False), ("uniform", 64, 1, 48, False),
    ("bisector", 1000, 2, 3, False), ("all_far", 1000, 2, 3, False), ("chain", 300, 2, 3, False),
    ("wide", 300, 3, 12, False), ("appended", 1000, 2, 12, False),
    ("uniform", 1000, 3, 3, True), ("appended", 1000, 3, 48, True), ("chain", 300, 2, 3, True),
    ("uniform", (1, 65, 1000), 3, 12, False), ("uniform", (1000, 1, 65), 3, 3, True),
    # SH rows of 1 and 2 floats: a 16-byte chunk of the copy then spans up to four rows
    ("uniform", 65, 2, 1, False), ("uniform", 1000, 2, 1, True), ("appended", 1000, 3, 1, True),
    ("uniform", 1000, 3, 2, True)]
IDS = [f"{k}-{'x'.join(map(str, n)) if isinstance(n, tuple) else n}-K{K}-sh{f}{'-shuffled' if s else ''}"
       for k, n, K, f, s in CASES]


def _t(chunk, dev=DEV):
    return tuple(torch.tensor(a, device=dev) for a in chunk)


def _gpu(chunks, cen, dev=DEV, **kw):
    out = H.merge_dynamic_hierarchies([_t(ch, dev) for ch in chunks], cen, **kw)
    assert all(o.is_cuda for o in out) and out[5].dtype == torch.int32 and out[6].dtype == torch.int32
    G = out[0].shape[0]
    assert out[1].shape == (G,) + tuple(chunks[0][1].shape[1:]) and out[2].shape == (G, 1)
    pos, shs, alpha, ls, rot, nodes, roots = [o.cpu().numpy() for o in out]
    return dict(pos=pos, shs=shs.reshape(G, -1), alpha=alpha.reshape(-1), log_scales=ls, rot=rot, nodes=nodes,
                chunk_roots=roots)


def _same(gpu, ref):
    np.testing.assert_array_equal(gpu["nodes"], ref["nodes"])
    np.testing.assert_array_equal(gpu["chunk_roots"], ref["chunk_roots"])
    for key in FLOATS:  # bits, so that -0.0 and NaN payloads count
        assert gpu[key].dtype == np.float32 and ref[key].dtype == np.float32
        np.testing.assert_array_equal(gpu[key].view(np.int32), ref[key].view(np.int32), err_msg=key)


@functools.lru_cache(maxsize=None)
def _scene(kind, L, K, shf, shuffle):
    chunks, cen = R.make_scene(kind, L, K, shf=shf, shuffle=shuffle)
    return chunks, cen, R.merge_ref(chunks, cen)


@pytest.mark.parametrize("kind,L,K,shf,shuffle", CASES, ids=IDS)
def test_merge_is_bit_exact(kind, L, K, shf, shuffle):
    chunks, cen, ref = _scene(kind, L, K, shf, shuffle)
    _same(_gpu(chunks, cen), ref)


@pytest.mark.parametrize("shf", [1, 2, 3, 4])
@pytest.mark.parametrize("phase", [0, 1, 2, 3])
def test_rows_whose_neighbours_trade_places(shf, phase):
    """Source rows like [5, 7, 6, 8]: the ends of a four-row run are consecutive in the source and the middle is not.
    With narrow rows one 16-byte chunk of the output spans such a run."""
    chunks, cen = R.make_scene("uniform", 65, 1, shf=shf)
    swapped = [R.middle_swapped(chunks[0], phase)]
    ref = R.merge_ref(swapped, cen)
    _, _, src = R.closed_form_nodes(swapped, cen)
    rows = src[1:, 1]
    ends_only = (rows[3:] - rows[:-3] == 3) & ((rows[1:-2] - rows[:-3] != 1) | (rows[2:-1] - rows[:-3] != 2))
    assert ends_only.sum() >= 20
    _same(_gpu(swapped, cen), ref)
    _same(_gpu(chunks, cen), ref)  # the same tree, stored in pre-order


def test_falloff_and_root_scale_are_arguments():
    chunks, cen, _ = _scene("uniform", 65, 2, 3, False)
    _same(_gpu(chunks, cen, falloff=0.2, root_scale=50.0), R.merge_ref(chunks, cen, falloff=0.2, root_scale=50.0))


def test_cpu_tensors_give_the_same_result():
    chunks, cen, ref = _scene("appended", 1000, 2, 12, False)
    _same(_gpu(chunks, cen, dev="cpu"), ref)
    _same(_gpu(chunks, torch.tensor(cen, device=DEV)), ref)


def test_one_chunk_in_preorder_is_the_identity_under_a_root():
    chunks, cen, _ = _scene("uniform", 1000, 1, 12, False)
    pos, shs, alpha, ls, rot, nodes = R.flat(chunks[0])
    out = _gpu(chunks, cen)
    n = len(nodes)
    assert len(out["nodes"]) == n + 1
    want = pos.copy()
    want[0] = cen[0]
    for got, inp in ((out["pos"], want), (out["shs"], shs), (out["alpha"], alpha), (out["log_scales"], ls),
                     (out["rot"], rot)):
        np.testing.assert_array_equal(got[1:].view(np.int32), inp.view(np.int32))
    nd = out["nodes"][1:]
    np.testing.assert_array_equal(nd[:, R.DEPTH], nodes[:, R.DEPTH] + 1)
    np.testing.assert_array_equal(nd[:, R.PARENT], nodes[:, R.PARENT] + 1)
    np.testing.assert_array_equal(nd[:, R.CHILD_COUNT], nodes[:, R.CHILD_COUNT])
    np.testing.assert_array_equal(nd[:, R.FIRST_CHILD], np.arange(n) + 2)
    inner = nodes[:, R.CHILD_COUNT] > 0
    np.testing.assert_array_equal(nd[inner, R.FIRST_CHILD], nodes[inner, R.FIRST_CHILD] + 1)
    np.testing.assert_array_equal(nd[:, R.NEXT_SIBLING], np.where(nodes[:, R.NEXT_SIBLING] > 0,
                                                                  nodes[:, R.NEXT_SIBLING] + 1, 0))
    leaf = ~inner
    np.testing.assert_array_equal(nd[leaf, R.MAX_SIDE], np.arange(leaf.sum()))
    assert np.all(nd[inner, R.MAX_SIDE] == -1)


def test_merging_a_merged_hierarchy_again():
    """The output of a K = 3 merge, scene root included, as the single chunk of a second merge: an n-ary input."""
    chunks, cen, ref = _scene("uniform", 1000, 3, 48, False)
    assert ref["nodes"][:, R.CHILD_COUNT].max() > 2
    first = H.merge_dynamic_hierarchies([_t(ch) for ch in chunks], cen)
    centre = np.array([[1.5, 1.0, 0.25]], np.float32)
    out = H.merge_dynamic_hierarchies([first[:6]], centre)
    again = R.merge_ref([tuple(ref[k] for k in ("pos", "shs", "alpha", "log_scales", "rot", "nodes"))], centre)
    got = [o.cpu().numpy() for o in out]
    G = len(got[0])
    _same(dict(pos=got[0], shs=got[1].reshape(G, -1), alpha=got[2].reshape(-1), log_scales=got[3], rot=got[4],
               nodes=got[5], chunk_roots=got[6]), again)
    assert G == len(ref["nodes"]) + 1


def test_nan_position_row_is_dropped_and_its_children_spliced():
    chunks, cen, _ = _scene("uniform", 65, 2, 3, False)
    pos, shs, alpha, ls, rot, nodes = chunks[0]
    w = R.weights(pos, 0, cen)
    kids = lambda i: R._children(nodes, i)  # noqa: E731
    hit = next(i for i in range(1, len(nodes)) if nodes[i, R.CHILD_COUNT] == 2 and w[i] > 0
               and all(w[c] > 0 for c in kids(i)))
    pos = pos.copy()
    pos[hit] = (np.nan, 1.0, 0.0)
    bad = [(pos, shs, alpha, ls, rot, nodes), chunks[1]]
    ref = R.merge_ref(bad, cen)
    assert len(ref["nodes"]) == len(R.merge_ref(chunks, cen)["nodes"]) - 1
    _same(_gpu(bad, cen), ref)


def test_nan_centre_raises():
    chunks, cen, _ = _scene("uniform", 65, 2, 3, False)
    for j in range(2):
        c = cen.copy()
        c[j, 1] = np.nan
        with pytest.raises(ValueError):
            _gpu(chunks, c)
    with pytest.raises(ValueError):
        _gpu(chunks, cen[:1])
    with pytest.raises(ValueError):  # chunks of different SH width
        _gpu([chunks[0], _scene("uniform", 65, 2, 12, False)[0][1]], cen)


def _break(nodes, what):
    nd = nodes.copy()
    n = len(nd)
    inner = np.where(nd[:, R.CHILD_COUNT] == 2)[0]
    a = inner[len(inner) // 2]
    c0 = nd[a, R.FIRST_CHILD]
    if what == "first_child_past_the_end":
        nd[a, R.FIRST_CHILD] = n + 5
    elif what == "first_child_huge":
        nd[a, R.FIRST_CHILD] = 2 ** 31 - 1
    elif what == "first_child_negative":
        nd[a, R.FIRST_CHILD] = -7
    elif what == "list_ends_early":
        nd[c0, R.NEXT_SIBLING] = 0
    elif what == "next_sibling_past_the_end":
        nd[c0, R.NEXT_SIBLING] = n
    elif what == "parent_names_another_node":
        nd[c0, R.PARENT] = inner[len(inner) // 2 - 1]
    elif what == "parent_out_of_range":
        nd[c0, R.PARENT] = n + 1
    elif what == "claimed_by_two_parents":
        # another row of a's depth lists a's first child as well
        b = next(i for i in inner if i != a and nd[i, R.DEPTH] == nd[a, R.DEPTH])
        nd[b, R.FIRST_CHILD] = c0
    elif what == "claimed_twice_by_one_list":
        nd[c0, R.NEXT_SIBLING] = c0
    elif what == "depth_off_by_one":
        nd[c0, R.DEPTH] += 1
    elif what == "depth_out_of_range":
        nd[:, R.DEPTH] += H.MERGE_MAX_DEPTH
    elif what == "child_count_too_large":
        nd[a, R.CHILD_COUNT] = n
    elif what == "root_listed_as_child":
        nd[c0, R.NEXT_SIBLING] = 0
        nd[a, R.FIRST_CHILD] = 0
    else:
        raise KeyError(what)
    return nd


@pytest.mark.parametrize("what", ["first_child_past_the_end", "first_child_huge", "first_child_negative",
                                  "list_ends_early", "next_sibling_past_the_end", "parent_names_another_node",
                                  "parent_out_of_range", "claimed_by_two_parents", "claimed_twice_by_one_list",
                                  "depth_off_by_one", "depth_out_of_range", "child_count_too_large",
                                  "root_listed_as_child"])
def test_malformed_links_raise_and_leave_the_next_call_correct(what):
    chunks, cen, ref = _scene("uniform", 65, 2, 3, False)
    bad = chunks[1][:5] + (_break(chunks[1][5], what),)
    with pytest.raises(ValueError):
        _gpu([chunks[0], bad], cen)
    _same(_gpu(chunks, cen), ref)


def test_runs_and_streams_agree_bitwise():
    chunks, cen, ref = _scene("appended", 1000, 3, 48, True)
    a, b = _gpu(chunks, cen), _gpu(chunks, cen)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        c = _gpu(chunks, cen)
    side.synchronize()
    stages = {}
    d = _gpu(chunks, cen, stage_ms=stages)
    assert set(stages) == set(H.MERGE_STAGES) and all(v >= 0 for v in stages.values())
    for other in (b, c, d):
        _same(other, a)
    _same(a, ref)


def test_lod_cut_of_the_merged_hierarchy_equals_the_oracle(monkeypatch):
    """expand_to_size_dynamic and get_interpolation_weights_dynamic on the K = 3 result for the three target sizes of
    tests/test_gpu_lod.py, with that file's comparison against the oracle."""
    import test_gpu_lod as TL
    chunks, cen, ref = _scene("uniform", 1000, 3, 48, False)
    out = _gpu(chunks, cen)
    _same(out, ref)
    h = dict(nodes=out["nodes"], means3D=out["pos"], scales=np.exp(out["log_scales"]))
    monkeypatch.setattr(TL, "_tree", lambda n=0, sky=0, seed=0: (h, None))
    TL.test_expand_to_size_dynamic_and_weights(0)
    # Those targets cut this scene near its leaves.  Three coarser ones, on which the oracle gives three different
    # cuts that select spliced nodes (more than two children) and children of such nodes: the same comparison.
    import gaussian_hierarchy as GH
    from oracle import oracle as O
    nodes, pos, sc = h["nodes"], h["means3D"], h["scales"]
    N = len(nodes)
    vp, vd = np.array([0.05, 0.0, -0.1], np.float32), np.array([0.0, 0.0, 1.0], np.float32)
    dv = lambda a: torch.tensor(a, device=DEV)  # noqa: E731
    sizes, wide, under_wide = [], 0, 0
    for target in (0.01, 0.03, 0.1):
        n_o, ri_o, pi_o, ni_o = O.expand_to_size_dynamic(nodes, pos, sc, target, vp, vd)
        ri, pi, ni = (torch.zeros(N, dtype=torch.int32, device=DEV) for _ in range(3))
        n = GH.expand_to_size_dynamic(dv(nodes), dv(pos), dv(sc), target, dv(vp), torch.tensor(vd), ri, pi, ni)
        assert n == n_o and n > 0
        for got, want in ((ri, ri_o), (ni, ni_o), (pi, pi_o)):
            np.testing.assert_array_equal(got[:n].cpu().numpy(), want[:n])
        ts, kids = torch.zeros(N, device=DEV), torch.zeros(N, dtype=torch.int32, device=DEV)
        GH.get_interpolation_weights_dynamic(ni[:n], target, dv(nodes), dv(pos), dv(sc), torch.tensor(vp),
                                             torch.tensor(vd), ts, kids)
        ts_o, kids_o = O.interp_weights_dynamic(ni_o[:n], target, nodes, pos, sc, vp)
        np.testing.assert_allclose(ts[:n].cpu().numpy(), ts_o, rtol=0, atol=1e-6)
        np.testing.assert_array_equal(kids[:n].cpu().numpy(), kids_o)
        sel = ni_o[:n]
        sizes.append(n_o)
        wide += int((nodes[sel, R.CHILD_COUNT] > 2).sum())
        par = nodes[sel, R.PARENT]
        under_wide += int((nodes[par[par >= 0], R.CHILD_COUNT] > 2).sum())
    assert len(set(sizes)) == 3 and wide > 0 and under_wide > 0


def test_merge_hierarchy_files_round_trip(tmp_path):
    import gaussian_hierarchy as GH
    chunks, cen, _ = _scene("uniform", 65, 3, 12, False)
    paths, cpaths, loaded = [], [], []
    for k, ch in enumerate(chunks):
        p = tmp_path / f"chunk{k}.dhier"
        GH.write_dynamic_hierarchy(str(p), *_t(ch, "cpu"), 1)
        c = tmp_path / f"center{k}.txt"
        c.write_text(" ".join(repr(float(v)) for v in cen[k]) + "\n")
        paths.append(str(p))
        cpaths.append(str(c))
        loaded.append(tuple(t.numpy() for t in GH.load_dynamic_hierarchy(str(p))))
    ref = R.merge_ref(loaded, cen)
    G = len(ref["nodes"])
    want = tmp_path / "want.dhier"
    GH.write_dynamic_hierarchy(str(want), torch.tensor(ref["pos"]), torch.tensor(ref["shs"].reshape(G, 4, 3)),
                               torch.tensor(ref["alpha"].reshape(G, 1)), torch.tensor(ref["log_scales"]),
                               torch.tensor(ref["rot"]), torch.tensor(ref["nodes"]), 1)
    for name, centers in (("paths.dhier", cpaths), ("array.dhier", cen)):
        got = tmp_path / name
        out = GH.merge_hierarchy_files(paths, centers, str(got), 1)
        assert out[6].cpu().tolist() == ref["chunk_roots"].tolist()
        assert got.read_bytes() == want.read_bytes()


def test_plan_reports_a_dropped_root_and_counts():
    """hlgs_hier_merge_plan on its own: the read-back block for a valid chunk, and the root bit for a NaN centre (which
    merge_dynamic_hierarchies rejects before it gets that far)."""
    from hlgs_core import _lib as L
    chunks, cen, ref = _scene("uniform", 65, 2, 3, False)
    pos, nodes = torch.tensor(chunks[0][0], device=DEV), torch.tensor(chunks[0][5], device=DEV)
    n = len(nodes)
    lib = L.load()
    scratch = torch.empty((lib.hlgs_hier_merge_scratch_size(n) + 256,), dtype=torch.uint8, device=DEV)
    scratch = scratch[-scratch.data_ptr() % 256:]
    for centers, status in ((cen, 0), (np.where(np.arange(2)[:, None] == 0, np.nan, cen).astype(np.float32), 2)):
        c = torch.tensor(centers, device=DEV)
        L.check(lib.hlgs_hier_merge_plan(n, 0, 2, L.ptr(c), L.ptr(pos), L.ptr(nodes), 0.05, L.ptr(scratch), 3,
                                         L.stream()))
        head = scratch[:4 * (8 + H.MERGE_MAX_DEPTH + 1)].view(torch.int32).cpu().numpy()
        assert head[0] == status
        np.testing.assert_array_equal(head[8:], np.bincount(chunks[0][5][:, R.DEPTH], minlength=H.MERGE_MAX_DEPTH + 1))
        if status == 0:
            assert head[1] == ref["chunk_roots"][1] - 1
            w = R.weights(np.concatenate([cen[:1], chunks[0][0][1:]]), 0, cen)
            assert head[2] == np.sum((w > 0) & (chunks[0][5][:, R.CHILD_COUNT] == 0))
