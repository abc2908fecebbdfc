"""The restatement of hlgs_core.activations.activate_regularized in torch float64 on the CPU: the activations of
scene/gaussian_model.py:44-56 and the two regularisers of train_post.py:565-576 over the n rows passed in.  Gradients
come from torch's autograd on this expression."""
import torch


def ref_inputs(n, device="cpu"):
    """The inputs of tests/test_gpu_act.py for n rows: seeded raw parameters with a saturated opacity and the zero
    rotation (normalize's eps branch) in row 0 and, past two rows, the opposite saturation and a rotation whose norm
    lies below the eps in row 1.  Returns (opacity_raw, scaling_raw, rotation_raw, generator)."""
    g = torch.Generator().manual_seed(n)
    op = torch.randn(n, 1, generator=g) * 4
    sc = torch.randn(n, 3, generator=g) * 2 - 4
    rot = torch.randn(n, 4, generator=g)
    if n:
        op[0] = 40.0
        rot[0] = 0.0
    if n > 2:
        op[1] = -40.0
        rot[1] = torch.tensor([1e-20, 0.0, 0.0, 0.0])
    return op.to(device), sc.to(device), rot.to(device), g


def activate_regularized_ref(opacity_raw, scaling_raw, rotation_raw):
    """(y, s, q, ol, sl) in float64: y = sigmoid(o), s = exp(sc), q = normalize(rot), ol = sum |y| / n,
    sl = sum |s| / n (the sum over 3 n values divided by n).  The inputs' own graph is kept: pass float64 leaves."""
    o, sc, rot = (t.double() for t in (opacity_raw, scaling_raw, rotation_raw))
    n = o.shape[0]
    y = torch.sigmoid(o)
    s = torch.exp(sc)
    q = torch.nn.functional.normalize(rot)
    ol = y.abs().sum() / n
    sl = s.abs().sum() / n
    return y, s, q, ol, sl


def leaves(*tensors):
    """Float64 CPU copies of the tensors that require grad."""
    return [t.detach().cpu().double().requires_grad_(True) for t in tensors]
