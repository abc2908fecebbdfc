"""The regularised activation pass (hlgs_core.activations.activate_regularized, csrc/act.hip: k_act_reg_fwd,
k_act_reg_bwd) against activate() and the float64 restatement of tests/act_reg_ref.py (train_post.py:565-576).

The sizes are the smallest at which each stage of the reduction can go wrong: one lane (1), the wave boundary (63, 64,
65), the workgroup boundary (255, 256, 257), and 300,001 rows = 1,172 workgroups, more partials than the reduce block's
1,024 threads, so that its strided loop runs twice.  Inputs are those of tests/test_gpu_act.py."""
import functools

import numpy as np
import pytest
import torch

import act_reg_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = [1, 63, 64, 65, 255, 256, 257, 300_001]


@functools.lru_cache(maxsize=None)
def _inputs(n):
    """(opacity_raw, scaling_raw, rotation_raw) on the device and the three upstream gradients drawn after them."""
    op, sc, rot, g = R.ref_inputs(n)
    ups = [torch.randn(s, generator=g) for s in ((n, 1), (n, 3), (n, 4))]
    return tuple(t.to(DEV) for t in (op, sc, rot)), tuple(u.to(DEV) for u in ups)


def _leaves(n):
    return [t.clone().requires_grad_(True) for t in _inputs(n)[0]]


@pytest.mark.parametrize("n", SIZES)
def test_forward(n):
    """The activated rows are activate()'s bit for bit; each loss is the sum of the call's own float32 rows over n.
    1e-6: all terms are positive, the workgroup tree over at most 768 float32 terms takes about ten roundings of 2^-24
    (6e-7), and the sum across workgroups is in double."""
    from hlgs_core.activations import activate, activate_regularized
    ins = _inputs(n)[0]
    got = activate_regularized(*ins)
    assert len(got) == 5
    for a, b in zip(got[:3], activate(*ins)):
        assert a.shape == b.shape and a.dtype == b.dtype
        assert torch.equal(a, b)
    for loss, rows, name in ((got[3], got[0], "opacity_loss"), (got[4], got[1], "scaling_loss")):
        assert loss.shape == () and loss.dtype == torch.float32 and loss.is_cuda
        want = float(rows.double().sum().cpu()) / n
        print(f"n={n} {name}: got {float(loss):.9g} want {want:.9g} rel {abs(float(loss) - want) / want:.2e}")
        assert abs(float(loss) - want) <= 1e-6 * want, (name, float(loss), want)


@pytest.mark.parametrize("n", SIZES)
def test_regularisers_only(n):
    """loss = 3 opacity_loss + 5 scaling_loss: the activated rows do not reach the loss, and the raw gradients are
    (3 / n) y (1 - y) and (5 / n) s of the returned rows."""
    from hlgs_core.activations import activate_regularized
    op, sc, rot = _leaves(n)
    y, s, _, ol, sl = activate_regularized(op, sc, rot)
    (3 * ol + 5 * sl).backward()
    yd, sd = y.detach().double(), s.detach().double()
    np.testing.assert_allclose(op.grad.cpu().numpy(), ((3 / n) * yd * (1 - yd)).cpu().numpy(), rtol=1e-6, atol=0)
    np.testing.assert_allclose(sc.grad.cpu().numpy(), ((5 / n) * sd).cpu().numpy(), rtol=1e-6, atol=0)
    assert rot.grad is None
    assert op.grad.shape == op.shape and sc.grad.shape == sc.shape


def test_opacity_loss_only_leaves_the_scaling_alone():
    from hlgs_core.activations import activate_regularized
    n = 257
    op, sc, rot = _leaves(n)
    y, _, _, ol, _ = activate_regularized(op, sc, rot)
    ol.backward()
    assert sc.grad is None and rot.grad is None
    yd = y.detach().double()
    np.testing.assert_allclose(op.grad.cpu().numpy(), (yd * (1 - yd) / n).cpu().numpy(), rtol=1e-6, atol=0)


@pytest.mark.parametrize("n", SIZES)
def test_combined_matches_restatement(n):
    """Random upstream gradients on the three activated outputs plus n opacity_loss + 2 n scaling_loss, against the
    restatement's autograd, with the two gradient criteria of test_activate_matches_torch.  The factor n makes the
    regularisers' share of a row's gradient of the order of the render's share: with a realistic lambda / n of about
    1e-5 it would lie below the tolerance, and a backward that drops it would pass."""
    from hlgs_core.activations import activate_regularized
    ups = _inputs(n)[1]
    ins = _leaves(n)
    got = activate_regularized(*ins)
    torch.autograd.backward(list(got[:3]) + [n * got[3] + 2 * n * got[4]], list(ups) + [None])
    ref_in = R.leaves(*ins)
    ref = R.activate_regularized_ref(*ref_in)
    torch.autograd.backward(list(ref[:3]) + [n * ref[3] + 2 * n * ref[4]], [u.cpu().double() for u in ups] + [None])
    for a, b, name in zip(ins, ref_in, ("opacity", "scaling", "rotation")):
        ga, gb = a.grad.cpu().double().numpy(), b.grad.numpy()
        assert ga.shape == gb.shape
        scale = np.abs(gb).max() + 1e-30
        print(f"n={n} {name}: max |diff| {np.abs(ga - gb).max():.3e} scale {scale:.3e}")
        assert np.abs(ga - gb).max() <= 1e-5 * scale, (name, np.abs(ga - gb).max(), scale)
        bad = np.abs(ga - gb) > 1e-4 * np.abs(gb) + 1e-6 * scale
        assert not bad.any(), (name, int(bad.sum()))


def test_deterministic():
    """Two calls on the same inputs give the same bits: no float atomics, a fixed summation order."""
    from hlgs_core.activations import activate_regularized
    n = 300_001
    ups = _inputs(n)[1]
    runs = []
    for _ in range(2):
        ins = _leaves(n)
        got = activate_regularized(*ins)
        torch.autograd.backward(list(got[:3]) + [n * got[3] + 2 * n * got[4]], list(ups) + [None])
        runs.append([got[3].detach(), got[4].detach()] + [t.grad for t in ins])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_no_rows():
    from hlgs_core.activations import activate_regularized
    ins = [torch.empty((0, w), device=DEV, requires_grad=True) for w in (1, 3, 4)]
    op, sc, rot, ol, sl = activate_regularized(*ins)
    assert op.shape == (0, 1) and sc.shape == (0, 3) and rot.shape == (0, 4)
    assert float(ol.detach()) == 0.0 and float(sl.detach()) == 0.0
    (op.sum() + sc.sum() + rot.sum() + ol + sl).backward()
    for t in ins:
        assert t.grad is not None and t.grad.shape == t.shape


def test_with_the_adam_step():
    """Four steps of loss = add_regularizers(0, ol, sl, 0.01, 0.02) alone through the dense Adam step on the opacity
    and the scaling (257 rows, 3 skybox rows), against oracle.spt_ref.adam_dense fed the restatement's gradients, with
    the tolerance of test_adam_step_matches_restatement.  The skybox rows stay where they are; the raw opacity of
    every other row falls at every step, which is what the densification round's dead threshold relies on.

    The learning rates are those train_post.py is run with (scripts/full_train.py:141-146: --opacity_lr 0.01
    --scaling_lr 0.001).  They also keep float32's own rounding inside the tolerance: the backward reads the float32 y,
    so 1 - y carries up to one ulp of y, 2^-24, whatever 1 - y is; that is (0.01 / n) 2^-24 on the gradient, and where
    |grad| is below Adam's eps (1e-8: y (1 - y) < 2.6e-4, |opacity_raw| > 8.3) a step moves by lr grad / eps, so four
    steps can differ from the float64 gradients' steps by 4 lr (0.01 / n) 2^-24 / 1e-8 = 9.3e-4 lr = 9.3e-6, within
    the 2e-6 * 8.3 = 1.7e-5 allowed there."""
    from hlgs_core.activations import activate_regularized
    from hlgs_core.mcmc import add_regularizers
    from hlgs_core.spt_cache import adam_step
    from oracle import spt_ref as SR
    n, sky, lrs = 257, 3, [0.01, 0.001]
    op0, sc0, rot = _inputs(n)[0]
    dp = [op0.clone().requires_grad_(True), sc0.clone().requires_grad_(True)]
    dm = [torch.zeros_like(p) for p in dp]
    dv = [torch.zeros_like(p) for p in dp]
    ps = [op0.cpu().clone(), sc0.cpu().clone()]
    ms = [torch.zeros_like(p) for p in ps]
    vs = [torch.zeros_like(p) for p in ps]
    start = [p.clone() for p in ps]
    for it in range(4):
        before = dp[0].detach().clone()
        for p in dp:
            p.grad = None
        _, _, _, ol, sl = activate_regularized(dp[0], dp[1], rot)
        add_regularizers(0.0, ol, sl, 0.01, 0.02).backward()
        with torch.no_grad():
            adam_step([p.data for p in dp], [p.grad for p in dp], dm, dv, lrs, it + 1, sky)
        assert bool((dp[0].detach()[sky:] < before[sky:]).all()), f"step {it}: an opacity did not fall"
        a, b, c = R.leaves(ps[0], ps[1], rot)
        _, _, _, rol, rsl = R.activate_regularized_ref(a, b, c)
        (0.01 * rol + 0.02 * rsl).backward()
        for p, gr, m, v, lr in zip(ps, (a.grad.float(), b.grad.float()), ms, vs, lrs):
            SR.adam_dense(p, gr, m, v, lr, it + 1, sky)
    for a, b in zip([p.detach() for p in dp] + dm + dv, ps + ms + vs):
        print(f"adam: max |diff| {float((a.cpu() - b).abs().max()):.3e}")
    for a, b in zip([p.detach() for p in dp] + dm + dv, ps + ms + vs):
        torch.testing.assert_close(a.cpu(), b, rtol=2e-6, atol=1e-7)
    for p, s in zip(dp, start):
        assert torch.equal(p.detach().cpu()[:sky], s[:sky])
