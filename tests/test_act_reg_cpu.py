"""The host side of the regularised activation pass (hlgs_core.activations.activate_regularized,
hlgs_core.mcmc.add_regularizers; train_post.py:565-576): the public signatures, the C ABI entries, the absence of a CPU
fallback, the weighting rule, and the float64 restatement (tests/act_reg_ref.py) against hand-computed values."""
import inspect
import math

import pytest
import torch

import act_reg_ref as R
from hlgs_core import _lib as L
from hlgs_core import mcmc
from hlgs_core.activations import activate_regularized

NEW_FUNCTIONS = {"hlgs_activate_reg_scratch_size": 1, "hlgs_activate_reg_forward": 10, "hlgs_activate_reg_backward": 12}


def test_signatures():
    assert list(inspect.signature(activate_regularized).parameters) == ["opacity_raw", "scaling_raw", "rotation_raw"]
    p = inspect.signature(mcmc.add_regularizers).parameters
    assert list(p) == ["loss", "opacity_loss", "scaling_loss", "lambda_opacity", "lambda_scaling"]
    assert p["lambda_opacity"].default == 0.01 and p["lambda_scaling"].default == 0.0


def test_abi_entries():
    lib = L.load()
    declared = L.header_functions()
    for name, nargs in NEW_FUNCTIONS.items():
        assert name in declared, name
        assert hasattr(lib, name), name
        assert len(L._SIGS[name][1]) == nargs, name
    assert L._SIGS["hlgs_activate_reg_scratch_size"][0] is L._sz
    # two float partials per workgroup of 256 rows, and room for n = 0
    sizes = [lib.hlgs_activate_reg_scratch_size(n) for n in (0, 1, 256, 257, 300_001, 50_000_000)]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:]))
    assert sizes[4] >= 8 * 1172 and sizes[5] >= 8 * 195_313


def test_cpu_tensors_raise():
    """There is no CPU fallback: host tensors raise with or without a device, the shape error first."""
    op, sc, rot, _ = R.ref_inputs(5)
    with pytest.raises(RuntimeError, match="HIP device|device tensors"):
        activate_regularized(op, sc, rot)
    with pytest.raises(RuntimeError, match="expected opacity"):
        activate_regularized(op, sc[:4], rot)


def test_add_regularizers_rule():
    loss = torch.tensor(0.25)
    ol, sl = torch.tensor(0.5), torch.tensor(float("inf"))
    got = mcmc.add_regularizers(loss, ol, sl)  # lambda_scaling = 0: the overflowed term is not added
    assert torch.isfinite(got) and float(got) == pytest.approx(0.25 + 0.01 * 0.5, rel=1e-6)
    assert mcmc.add_regularizers(loss, ol, sl, 0.0, 0.0) is loss
    got = mcmc.add_regularizers(loss, ol, torch.tensor(2.0), 0.02, 0.5)
    assert float(got) == pytest.approx(0.25 + 0.02 * 0.5 + 0.5 * 2.0, rel=1e-6)
    assert float(mcmc.add_regularizers(loss, ol, torch.tensor(2.0), 0.0, 0.5)) == pytest.approx(1.25, rel=1e-6)


def test_restatement_by_hand():
    """n = 2: o = (0, ln 3), scales = ln of (1, 2, 3) and (4, 5, 6), rotations (3, 0, 4, 0) and (0, 0, 0, 2)."""
    o = torch.tensor([[0.0], [math.log(3.0)]], dtype=torch.float64)
    sc = torch.log(torch.tensor([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]], dtype=torch.float64))
    rot = torch.tensor([[3.0, 0.0, 4.0, 0.0], [0.0, 0.0, 0.0, 2.0]], dtype=torch.float64)
    a, b, c = R.leaves(o, sc, rot)
    y, s, q, ol, sl = R.activate_regularized_ref(a, b, c)
    close = lambda x, want: torch.testing.assert_close(x, torch.tensor(want, dtype=torch.float64), rtol=1e-12, atol=0)  # noqa: E731
    close(y.detach(), [[0.5], [0.75]])
    close(s.detach(), [[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]])
    close(q.detach(), [[0.6, 0.0, 0.8, 0.0], [0.0, 0.0, 0.0, 1.0]])
    close(ol.detach(), (0.5 + 0.75) / 2)
    close(sl.detach(), 21.0 / 2)  # the sum over 3 n values divided by n
    (3 * ol + 5 * sl).backward()
    close(a.grad, [[1.5 * 0.5 * 0.5], [1.5 * 0.75 * 0.25]])  # (3 / n) y (1 - y)
    close(b.grad, [[2.5, 5.0, 7.5], [10.0, 12.5, 15.0]])     # (5 / n) s
    assert c.grad is None


def test_ref_inputs_plant_the_edge_rows():
    op, sc, rot, _ = R.ref_inputs(257)
    assert float(op[0]) == 40.0 and float(op[1]) == -40.0
    assert not rot[0].any() and float(rot[1].norm()) < 1e-12
    op1, _, rot1, _ = R.ref_inputs(1)
    assert float(op1[0]) == 40.0 and not rot1[0].any()
