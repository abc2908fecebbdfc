"""The host side of the adaptive density control (hlgs_core/densify.py, csrc/density.hip): the C ABI of the new
section of include/hlgs.h, the sizing query, the optimizer rebinding on a CPU Adam, the float64 restatement's own
properties on the test recipe, and the absence of a CPU fallback."""
import ctypes as C

import pytest
import torch

import densify_ref as R
from hlgs_core import _lib as L
from hlgs_core import densify as D

NEW_FUNCTIONS = ["hlgs_density_stats", "hlgs_density_select", "hlgs_densify_scratch_size", "hlgs_densify_plan",
                 "hlgs_densify_emit", "hlgs_opacity_reset"]


def test_header_declares_and_library_exports_the_entry_points():
    lib = L.load()
    declared = L.header_functions()
    for name in NEW_FUNCTIONS:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in L._SIGS, name


def test_scratch_size_is_monotone_and_non_zero():
    lib = L.load()
    sizes = [lib.hlgs_densify_scratch_size(P) for P in (0, 1, 255, 257, 2048, 2049, 100_003, 1_000_000, 4_000_000)]
    assert sizes[0] > 0
    assert all(a <= b for a, b in zip(sizes, sizes[1:]))
    assert sizes[1] < sizes[-1]
    # two scans and two row lists of 4 bytes per row, at least
    assert sizes[-1] >= 16 * 4_000_000


def _c_layout(struct, fields):
    """sizeof and field offsets of a header struct, as gcc lays it out from include/hlgs.h itself."""
    import os
    import subprocess
    import tempfile
    body = "".join(f'printf("%zu\\n", offsetof({struct}, {f}));' for f in fields)
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "hlgs.h"\n'
           f'int main(void) {{ printf("%zu\\n", sizeof({struct})); {body} return 0; }}\n')
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.dirname(L.HEADER), c, "-o", exe])
        vals = [int(v) for v in subprocess.check_output([exe]).split()]
    return vals[0], vals[1:]


def test_densify_table_matches_header_layout():
    names = [f[0] for f in L.DensifyTable._fields_]
    size, offs = _c_layout("hlgs_densify_table", names)
    assert C.sizeof(L.DensifyTable) == size
    assert [getattr(L.DensifyTable, n).offset for n in names] == offs


def test_mode_and_role_codes_match_header():
    import re
    txt = open(L.HEADER).read()
    code = lambda name: int(re.search(rf"#define HLGS_DENSIFY_{name} (\d+)", txt).group(1))  # noqa: E731
    assert {k: code(k.upper()) for k in L.DENSIFY_MODES} == L.DENSIFY_MODES
    assert [code(n) for n in ("COPY", "ZERO", "XYZ", "SCALING", "OPACITY")] == [
        L.DENSIFY_COPY, L.DENSIFY_ZERO, L.DENSIFY_XYZ, L.DENSIFY_SCALING, L.DENSIFY_OPACITY]


# ---------------------------------------------------------------------------------------------- rebind_optimizer
def _adam(params):
    groups = [{"params": [torch.nn.Parameter(params[k].clone())], "lr": 1e-2, "name": k} for k in R.NAMES]
    opt = torch.optim.Adam(groups, lr=0.0, eps=1e-15)
    for g in opt.param_groups:
        g["params"][0].grad = torch.ones_like(g["params"][0])
    opt.step()
    return opt


def test_rebind_optimizer_replaces_parameters_and_carries_moments():
    P = 37
    inp = R.recipe(P, sh_rest=9)
    opt = _adam(inp["params"])
    old = {g["name"]: g["params"][0] for g in opt.param_groups}
    state = {k: opt.state[old[k]] for k in R.NAMES}
    sel = torch.zeros(P, dtype=torch.bool)
    sel[[3, 4, 20]] = True
    prune = torch.zeros(P, dtype=torch.bool)
    prune[[0, 11]] = True
    params = {k: old[k].detach() for k in R.NAMES}
    m = {k: state[k]["exp_avg"] for k in R.NAMES}
    v = {k: state[k]["exp_avg_sq"] for k in R.NAMES}
    stats = (inp["grad_accum"], inp["denom"], inp["max_radii2D"])
    p2, m2, v2, _ = R.densify_and_prune(params, m, v, stats, sel, prune, mode="clone", dtype=torch.float32)
    n_kept, n_new = P - 2, 6
    new = D.rebind_optimizer(opt, p2, m2, v2)
    assert set(new) == set(R.NAMES)
    kept = (~prune).nonzero().reshape(-1)
    for g in opt.param_groups:
        k = g["name"]
        p = g["params"][0]
        assert p is new[k] and p is not old[k] and isinstance(p, torch.nn.Parameter) and p.requires_grad
        assert p.shape[0] == n_kept + n_new and torch.equal(p.detach(), p2[k])
        assert old[k] not in opt.state
        st = opt.state[p]
        assert float(st["step"]) == 1
        for key, before in (("exp_avg", m[k]), ("exp_avg_sq", v[k])):
            assert torch.equal(st[key][:n_kept], before[kept])
            assert st[key][:n_kept].abs().sum() > 0 or before.numel() == 0
            assert not st[key][n_kept:].any()
    for g in opt.param_groups:
        g["params"][0].grad = torch.ones_like(g["params"][0])
    before = {k: new[k].detach().clone() for k in R.NAMES}
    opt.step()
    for k in R.NAMES:
        assert float(opt.state[new[k]]["step"]) == 2
        assert not torch.equal(new[k].detach(), before[k])


def test_rebind_optimizer_subset_without_state_and_unknown_name():
    inp = R.recipe(5, sh_rest=0)
    groups = [{"params": [torch.nn.Parameter(inp["params"][k].clone())], "lr": 1e-2, "name": k} for k in R.NAMES]
    opt = torch.optim.Adam(groups, lr=0.0)
    t = torch.zeros(7, 1)
    new = D.rebind_optimizer(opt, {"opacity": t}, {"opacity": t.clone()}, {"opacity": t.clone()})
    assert list(new) == ["opacity"] and len(opt.state) == 0  # no step taken: no state to carry (:1310-1312)
    assert opt.param_groups[3]["params"][0] is new["opacity"]
    with pytest.raises(RuntimeError, match="no group named"):
        D.rebind_optimizer(opt, {"colour": t})


# ---------------------------------------------------------------------------------------------- the restatement
def test_recipe_is_decided_far_from_its_thresholds():
    """On the recipe at P = 100,003 the float64 rule selects 12,286 and prunes 4,427 rows; no row lies within a
    relative 1e-5 of a threshold, and torch's float32 evaluation makes the same decisions -- so the cap of 8 excused
    rows in the GPU test cannot hide a failure."""
    P = 100_003
    inp = R.recipe(P, sh_rest=0)
    a = (inp["grad_accum"], inp["max_radii2D"], inp["params"]["opacity"])
    sel, prune, near = R.select_masks(*a)
    print(f"recipe P={P}: selected {int(sel.sum())}, pruned {int(prune.sum())}, near {int(near.sum())}")
    assert (int(sel.sum()), int(prune.sum())) == (12_286, 4_427)
    assert int(near.sum()) == 0
    sel32, prune32, _ = R.select_masks(*a, dtype=torch.float32)
    assert torch.equal(sel, sel32) and torch.equal(prune, prune32)
    assert not (sel & prune).any()
    assert not sel[inp["grad_accum"].reshape(-1).isnan()].any()


def test_prune_then_append_equals_append_then_prune():
    """A new row of the shrink mode has opacity >= 0.15 / (0.8 N) > 0.005, so the reference's prune mask evaluated on
    the grown table never reaches a new row: pruning the old rows first is the same table."""
    P = 4099
    inp = R.recipe(P, sh_rest=0)
    sel, prune, _ = R.select_masks(inp["grad_accum"], inp["max_radii2D"], inp["params"]["opacity"])
    for N in (2, 3):
        new = R.new_rows(inp["params"], sel, "shrink", N)
        assert float(torch.sigmoid(new["opacity"]).min()) >= 0.15 / (0.8 * N) > 0.005


# ---------------------------------------------------------------------------------------------- no CPU fallback
def test_no_cpu_fallback():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    P = 9
    inp = R.recipe(P, sh_rest=9)
    stats = D.DensityStats(P, "cpu")
    with pytest.raises(RuntimeError, match="HIP device"):
        stats.update_(torch.zeros(P, 3), torch.ones(P, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="HIP device"):
        D.select(stats, inp["params"]["opacity"], 0.015)
    sel = torch.ones(P, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="HIP device"):
        D.densify_and_prune(inp["params"], inp["exp_avg"], inp["exp_avg_sq"], stats, sel, seed=1)
    with pytest.raises(RuntimeError, match="HIP device"):
        D.reset_opacity_(inp["params"]["opacity"], inp["exp_avg"]["opacity"], inp["exp_avg_sq"]["opacity"])
    # the shape errors come first
    with pytest.raises(RuntimeError, match="radii must be"):
        stats.update_(torch.zeros(P, 3), torch.ones(P + 1, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="opacity_raw must be"):
        D.select(stats, torch.zeros(P + 1, 1), 0.015)
    with pytest.raises(RuntimeError, match="mode must be"):
        D.densify_and_prune(inp["params"], inp["exp_avg"], inp["exp_avg_sq"], stats, sel, mode="merge", seed=1)
    with pytest.raises(RuntimeError, match="select must be"):
        D.densify_and_prune(inp["params"], inp["exp_avg"], inp["exp_avg_sq"], stats, sel[:-1], seed=1)
    with pytest.raises(RuntimeError, match="exp_avg must be"):
        D.reset_opacity_(inp["params"]["opacity"], torch.zeros(P + 1, 1), inp["exp_avg_sq"]["opacity"])
