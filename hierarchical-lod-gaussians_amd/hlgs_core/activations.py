"""The parameter activations of the training step on the HIP path (libhlgs.so, csrc/act.hip).

    activate(opacity_raw, scaling_raw, rotation_raw) -> (opacity, scales, rotations)

is GaussianModel.get_opacity / get_scaling / get_rotation (scene/gaussian_model.py:44-56: sigmoid, exp,
torch.nn.functional.normalize) over every resident row in one kernel, and their backward in one more; torch runs
them as about ten elementwise and reduction kernels per step (train_post.py's render of the cached rows).

    activate_regularized(opacity_raw, scaling_raw, rotation_raw)
        -> (opacity, scales, rotations, opacity_loss, scaling_loss)

is the same pass with the two regularisers of the MCMC training step (train_post.py:565-576) reduced beside it:
opacity_loss = sum |opacity| / n and scaling_loss = sum |scales| / n over the n rows passed in;
hlgs_core.mcmc.add_regularizers adds them to the loss.
"""
import torch

from hlgs_core import _lib as L


def _raw_rows(op_raw, sc_raw, rot_raw):
    n = op_raw.shape[0]
    if sc_raw.shape != (n, 3) or rot_raw.shape != (n, 4) or op_raw.numel() != n:
        raise RuntimeError("activate: expected opacity (n, 1), scaling (n, 3) and rotation (n, 4) rows")
    rows = tuple(t.detach().contiguous().float() for t in (op_raw, sc_raw, rot_raw))
    L.require_gpu(*rows)
    return (n,) + rows


class _Activate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, op_raw, sc_raw, rot_raw):
        n, o_r, s_r, r_r = _raw_rows(op_raw, sc_raw, rot_raw)
        op, sc, rot = torch.empty_like(o_r), torch.empty_like(s_r), torch.empty_like(r_r)
        L.check(L.load().hlgs_activate_forward(n, L.ptr(o_r), L.ptr(s_r), L.ptr(r_r), L.ptr(op), L.ptr(sc),
                                               L.ptr(rot), L.stream()))
        ctx.save_for_backward(op, sc, r_r)
        ctx.set_materialize_grads(False)
        return op.view(op_raw.shape), sc, rot

    @staticmethod
    def backward(ctx, g_op, g_sc, g_rot):
        op, sc, r_r = ctx.saved_tensors
        n = r_r.shape[0]
        g = [None if t is None else t.contiguous().float() for t in (g_op, g_sc, g_rot)]
        d = [None if t is None else torch.empty_like(s) for t, s in zip(g, (op, sc, r_r))]
        L.check(L.load().hlgs_activate_backward(n, L.ptr(op), L.ptr(sc), L.ptr(r_r), *(L.ptr(t) for t in g),
                                                *(L.ptr(t) for t in d), L.stream()))
        if d[0] is not None:
            d[0] = d[0].view(op.shape)
        return tuple(d)


class _ActivateReg(torch.autograd.Function):
    """_Activate with a fourth output reg = (opacity_loss, scaling_loss), a (2,) device tensor, so that the upstream
    gradient of both losses arrives as one (2,) device tensor and goes to the kernel as it is (no host read).  The
    fifth output is a host list of two flags that _PickLoss sets during a backward pass: which of the two losses
    reached the loss is a fact of the graph, known on the host, and it decides whether a raw tensor whose activated
    output got no gradient receives one (as torch's own expression would) or None."""

    @staticmethod
    def forward(ctx, op_raw, sc_raw, rot_raw):
        n, o_r, s_r, r_r = _raw_rows(op_raw, sc_raw, rot_raw)
        lib = L.load()
        op, sc, rot = torch.empty_like(o_r), torch.empty_like(s_r), torch.empty_like(r_r)
        reg = torch.empty((2,), dtype=torch.float32, device=o_r.device)
        scratch = torch.empty((lib.hlgs_activate_reg_scratch_size(n),), dtype=torch.uint8, device=o_r.device)
        L.check(lib.hlgs_activate_reg_forward(n, L.ptr(o_r), L.ptr(s_r), L.ptr(r_r), L.ptr(op), L.ptr(sc), L.ptr(rot),
                                              L.ptr(reg), L.ptr(scratch), L.stream()))
        ctx.save_for_backward(op, sc, r_r)
        ctx.set_materialize_grads(False)
        ctx.reg_used = [False, False]
        return op.view(op_raw.shape), sc, rot, reg, ctx.reg_used

    @staticmethod
    def backward(ctx, g_op, g_sc, g_rot, g_reg, _):
        op, sc, r_r = ctx.saved_tensors
        n = r_r.shape[0]
        used, ctx.reg_used[:] = list(ctx.reg_used), [False, False]  # cleared for a later pass over a retained graph
        g = [None if t is None else t.contiguous().float() for t in (g_op, g_sc, g_rot, g_reg)]
        # the kernel adds g_reg / n to both tensors' gradients (the unused loss's entry is 0) and writes both
        d = [torch.empty_like(s) if t is not None or (g[3] is not None and k < 2) else None
             for k, (t, s) in enumerate(zip(g[:3], (op, sc, r_r)))]
        L.check(L.load().hlgs_activate_reg_backward(n, L.ptr(op), L.ptr(sc), L.ptr(r_r), *(L.ptr(t) for t in g),
                                                    *(L.ptr(t) for t in d), L.stream()))
        for k in range(2):  # reached by neither its activated output nor its loss: no gradient, not zeros
            if g[k] is None and not used[k]:
                d[k] = None
        if d[0] is not None:
            d[0] = d[0].view(op.shape)
        return tuple(d)


class _PickLoss(torch.autograd.Function):
    """reg[idx] as a 0-dim tensor; its backward places the upstream gradient in a (2,) tensor and notes on the host
    that this loss was reached."""

    @staticmethod
    def forward(ctx, reg, idx, used):
        ctx.idx, ctx.used = idx, used
        return reg[idx]

    @staticmethod
    def backward(ctx, g):
        ctx.used[ctx.idx] = True
        return torch.nn.functional.pad(g.reshape(1), (ctx.idx, 1 - ctx.idx)), None, None


def activate(opacity_raw, scaling_raw, rotation_raw):
    """(sigmoid(opacity_raw), exp(scaling_raw), normalize(rotation_raw)) in one HIP pass, differentiable."""
    return _Activate.apply(opacity_raw, scaling_raw, rotation_raw)


def activate_regularized(opacity_raw, scaling_raw, rotation_raw):
    """activate() and, from the same pass, the regularisers of train_post.py:565-576 over the n rows passed in:
    returns (opacity, scales, rotations, opacity_loss, scaling_loss) with opacity_loss = sum |opacity| / n and
    scaling_loss = sum |scales| / n (the sum over 3 n values divided by n, as the reference does), both 0-dim float32
    device tensors with autograd; n = 0 gives (0, 0).  The first three results are activate()'s bit for bit.  Pass
    every resident row, skybox rows included, as len(render_indices) counts them.  The losses are the same from run
    to run (no float atomics).  opacity_loss and scaling_loss / 3 are also the "Mean Opacity" and "Mean Scaling"
    train_post.py:659-660 logs."""
    op, sc, rot, reg, used = _ActivateReg.apply(opacity_raw, scaling_raw, rotation_raw)
    return op, sc, rot, _PickLoss.apply(reg, 0, used), _PickLoss.apply(reg, 1, used)
