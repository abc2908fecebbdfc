"""The exposure / clamp / alpha-mask path of photometric_loss and image_metrics (csrc/loss.hip's post kernels) against
the float64 CPU composition the reference runs between its rasterizer and its loss: the exposure expression of
gaussian_renderer/__init__.py:139-141, .clamp(0, 1) (:142), * alpha_mask (train_single.py:102-104), then
oracle/loss_ref.photometric, with autograd for d image and dE.

Bounds are those of tests/test_gpu_loss.py: loss within 1e-5 relative, gradients within 1e-4 of the reference
gradient's largest magnitude (dE: of max |dE_ref| over its 12 entries), d invdepth within 1e-6.

Inputs: E = eye(3, 4) + 0.15 randn on the 3x3 block + 0.05 randn bias; target pre-clamp values t ~ U(-0.3, 1.3) with
every value within 1e-3 of 0 or 1 moved by +4e-3; raw = (t - b) A^-1 in float64, cast to float32.  Every pre-clamp
value then stays clear of the clamp edges, so float32 and float64 gate the same pixels and no pixel is left out of the
comparison.  gt is premultiplied by the mask (scene/cameras.py:73-74)."""
import functools

import numpy as np
import pytest
import torch

from oracle import loss_ref as LR

pytestmark = pytest.mark.gpu
DEV = "cuda"
LAM = 0.2


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _mask(kind, H, W, g):
    if kind is None:
        return None
    if kind == "binary":  # the train_test_exp layout (scene/cameras.py:64-67): left half zero
        m = torch.ones(1, H, W)
        m[..., :W // 2] = 0
        return m
    return torch.rand(1, H, W, generator=g)  # soft, in [0, 1]


def _expose(x, E):
    """The reference's expression (gaussian_renderer/__init__.py:139-141)."""
    return torch.matmul(x.permute(1, 2, 0), E[:3, :3]).permute(2, 0, 1) + E[:3, 3, None, None]


@functools.lru_cache(maxsize=None)
def _case(shape, mask_kind, expo, clamp, depth=False):
    """Seeded float32 inputs and the float64 CPU reference of one case; computed once, shared, never modified."""
    _, H, W = shape
    g = torch.Generator().manual_seed(H * 1000 + W + (0 if mask_kind is None else len(mask_kind)))
    E = None
    t = torch.rand(shape, generator=g, dtype=torch.float64) * 1.6 - 0.3
    near = ((t.abs() < 1e-3) | ((t - 1).abs() < 1e-3))
    t = torch.where(near, t + 4e-3, t)
    raw = t
    if expo:
        E = torch.eye(3, 4, dtype=torch.float64)
        E[:, :3] += 0.15 * torch.randn(3, 3, generator=g, dtype=torch.float64)
        E[:, 3] += 0.05 * torch.randn(3, generator=g, dtype=torch.float64)
        E = E.float()  # what the kernel receives; the reference uses these values in float64
        A, b = E[:, :3].double(), E[:, 3].double()
        raw = ((t.permute(1, 2, 0) - b) @ torch.linalg.inv(A)).permute(2, 0, 1)
    raw = raw.float().contiguous()
    m = _mask(mask_kind, H, W, g)
    gt = torch.rand(shape, generator=g)
    if m is not None:
        gt = gt * m
    dep = None
    if depth:
        dep = (torch.rand(1, H, W, generator=g), torch.rand(1, H, W, generator=g),
               (torch.rand(1, H, W, generator=g) > 0.3).float())
    # float64 reference
    x = raw.double().requires_grad_(True)
    Ed = E.double().requires_grad_(True) if expo else None
    pre = _expose(x, Ed) if expo else x
    img = pre.clamp(0, 1) if clamp else pre
    if m is not None:
        img = img * m.double()
    inv = dep[0].double().requires_grad_(True) if depth else None
    loss = LR.photometric(img, gt, LAM, inv, dep[1] if depth else None, dep[2] if depth else None,
                          0.5 if depth else 0.0)
    wrt = [x] + ([Ed] if expo else []) + ([inv] if depth else [])
    grads = list(torch.autograd.grad(loss, wrt))
    loss, img = loss.detach(), img.detach()
    ref = dict(loss=float(loss), l1=float((img - gt.double()).abs().mean()), ssim=float(LR.ssim(img, gt)),
               pre=pre.detach(), d_img=grads.pop(0).numpy(), d_E=grads.pop(0).numpy() if expo else None,
               d_inv=grads.pop(0).numpy() if depth else None)
    # the construction: no pre-clamp value sits where float32 and float64 could gate differently
    edge = torch.minimum(ref["pre"].abs(), (ref["pre"] - 1).abs()).min()
    assert float(edge) >= 5e-4, float(edge)
    return dict(raw=raw, gt=gt, E=E, m=m, dep=dep, clamp=clamp, ref=ref)


def _run(c, image_grad=True, expo_grad=True):
    """photometric_loss on the case's inputs -> (outputs, image, exposure, invdepth) after backward."""
    from hlgs_core.loss import photometric_loss
    img = c["raw"].to(DEV).requires_grad_(image_grad)
    E = c["E"].to(DEV).requires_grad_(expo_grad) if c["E"] is not None else None
    m = c["m"].to(DEV) if c["m"] is not None else None
    kw = {}
    inv = None
    if c["dep"] is not None:
        inv = c["dep"][0].to(DEV).requires_grad_(True)
        kw = dict(invdepth=inv, mono_invdepth=c["dep"][1].to(DEV), depth_mask=c["dep"][2].to(DEV), depth_weight=0.5)
    out = photometric_loss(img, c["gt"].to(DEV), LAM, clamp_image=c["clamp"], exposure=E, alpha_mask=m, **kw)
    out[0].backward()
    return out, img, E, inv


SHAPES = [(3, 7, 9), (3, 45, 133), (3, 33, 260), (3, 70, 90)]
CASES = ([(s, k, True, True) for s in SHAPES for k in ("binary", "soft")]
         + [((3, 7, 9), None, True, True), ((3, 45, 133), None, True, True)]       # exposure without a mask
         + [((3, 33, 260), "binary", False, True), ((3, 45, 133), "soft", False, True)]  # a mask without exposure
         + [((3, 70, 90), "soft", True, False)])                                  # clamp off


@pytest.mark.parametrize("shape,mask_kind,expo,clamp", CASES)
def test_exposure_mask_loss_and_gradients_match_float64_composition(shape, mask_kind, expo, clamp):
    c = _case(shape, mask_kind, expo, clamp)
    ref = c["ref"]
    (tot, Ll1, ssim_v, _), img, E, _ = _run(c)
    tot = tot.detach()
    d_img = img.grad.cpu().numpy()
    print(f"loss rel {abs(float(tot) - ref['loss']) / abs(ref['loss']):.3e}  d_img {_rel(d_img, ref['d_img']):.3e}",
          f" dE {_rel(E.grad.cpu().numpy(), ref['d_E']):.3e}" if expo else "")
    assert abs(float(tot.detach()) - ref["loss"]) <= 1e-5 * abs(ref["loss"])
    assert abs(float(Ll1) - ref["l1"]) <= 1e-5 * abs(ref["l1"])      # the by-products are those of the
    assert abs(float(ssim_v) - ref["ssim"]) <= 1e-5 * abs(ref["ssim"])  # transformed image
    assert _rel(d_img, ref["d_img"]) <= 1e-4
    if expo:
        assert E.grad.shape == (3, 4)
        assert _rel(E.grad.cpu().numpy(), ref["d_E"]) <= 1e-4
        assert np.abs(ref["d_E"]).min() >= 0.01 * np.abs(ref["d_E"]).max()  # every entry carries weight in the bound


def test_exposure_mask_with_depth_term():
    c = _case((3, 45, 133), "soft", True, True, True)
    ref = c["ref"]
    (tot, _, _, _), img, E, inv = _run(c)
    assert abs(float(tot.detach()) - ref["loss"]) <= 1e-5 * abs(ref["loss"])
    assert _rel(img.grad.cpu().numpy(), ref["d_img"]) <= 1e-4
    assert _rel(E.grad.cpu().numpy(), ref["d_E"]) <= 1e-4
    assert _rel(inv.grad.cpu().numpy(), ref["d_inv"]) <= 1e-6


@pytest.mark.parametrize("clamp", [True, False])
def test_identity_exposure_and_unit_mask_are_free(clamp):
    """exposure = eye(3, 4) and a mask of ones: 1 x + 0 y + 0 z + 0 and 1 x are exact, so the image gradient equals the
    plain path's bit for bit; any difference would be a reordered chain."""
    from hlgs_core.loss import photometric_loss
    g = torch.Generator().manual_seed(7)
    img = (torch.rand(3, 70, 90, generator=g) * 1.6 - 0.3).to(DEV)  # ~35% of the values outside [0, 1]
    gt = torch.rand(3, 70, 90, generator=g).to(DEV)
    a = img.clone().requires_grad_(True)
    b = img.clone().requires_grad_(True)
    E = torch.eye(3, 4, device=DEV, requires_grad=True)
    la = photometric_loss(a, gt, LAM, clamp_image=clamp, exposure=E, alpha_mask=torch.ones(1, 70, 90, device=DEV))[0]
    lb = photometric_loss(b, gt, LAM, clamp_image=clamp)[0]
    la.backward()
    lb.backward()
    assert abs(float(la.detach()) - float(lb.detach())) <= 1e-6 * abs(float(lb.detach()))
    assert torch.equal(a.grad, b.grad)
    assert torch.isfinite(E.grad).all()


def test_gradient_is_zero_under_the_mask_and_outside_the_clamp():
    c = _case((3, 45, 133), "binary", True, True)
    _, img, _, _ = _run(c)
    pre = c["ref"]["pre"]
    # d raw mixes the channels: a pixel's gradient is zero when the mask is zero, or when all three channels are gated
    masked = (c["m"] == 0).expand(3, -1, -1)
    assert masked.any() and (img.grad.cpu()[masked] == 0).all()
    gated_all = ((pre < 0) | (pre > 1)).all(0, keepdim=True).expand(3, -1, -1)
    assert gated_all.any() and (img.grad.cpu()[gated_all] == 0).all()
    # without the exposure the gate is per value
    c = _case((3, 45, 133), "soft", False, True)
    _, img, _, _ = _run(c)
    out = (c["raw"] < 0) | (c["raw"] > 1)
    assert 0.3 < float(out.float().mean()) < 0.45
    assert (img.grad.cpu()[out] == 0).all()
    assert (img.grad.cpu()[~out & (c["m"] > 0.05).expand(3, -1, -1)] != 0).any()


def test_two_runs_are_bitwise_equal():
    c = _case((3, 33, 260), "soft", True, True)
    (t0, _, _, _), i0, E0, _ = _run(c)
    (t1, _, _, _), i1, E1, _ = _run(c)
    assert float(t0.detach()) == float(t1.detach())
    assert torch.equal(i0.grad, i1.grad)
    assert torch.equal(E0.grad, E1.grad)


def test_exposure_gradient_is_optional_and_stands_alone():
    c = _case((3, 45, 133), "soft", True, True)
    _, i0, E0, _ = _run(c)
    _, i1, E1, _ = _run(c, expo_grad=False)  # no exposure gradient: the same d image
    assert E1.grad is None
    assert torch.equal(i0.grad, i1.grad)
    _, i2, E2, _ = _run(c, image_grad=False)  # only the exposure requires grad
    assert i2.grad is None
    assert torch.equal(E2.grad, E0.grad)


@pytest.mark.parametrize("masked", [False, True])
def test_image_metrics_match_reference_psnr_and_ssim(masked):
    from hlgs_core.loss import image_metrics
    g = torch.Generator().manual_seed(11)
    raw = torch.rand(3, 45, 133, generator=g) * 1.6 - 0.3
    m = torch.rand(1, 45, 133, generator=g) if masked else None
    gt = torch.rand(3, 45, 133, generator=g)
    raw[1] = gt[1] + 0.05 * torch.randn(45, 133, generator=g)  # unequal plane errors: the two PSNR groupings differ
    if masked:
        gt = gt * m

    def psnr(a, b):  # utils/image_utils.py:17-19
        mse = ((a - b) ** 2).view(a.shape[0], -1).mean(1, keepdim=True)
        return 20 * torch.log10(1.0 / torch.sqrt(mse))

    vals = []
    for lead in ((), (1,)):
        img = raw.double().clamp(0, 1) * (m.double() if masked else 1.0)
        a, b = img.reshape(lead + img.shape), gt.double().reshape(lead + gt.shape)
        got = image_metrics(raw.reshape(lead + raw.shape).to(DEV), gt.reshape(lead + gt.shape).to(DEV),
                            alpha_mask=m.to(DEV) if masked else None)
        ref_mse = ((img - gt.double()) ** 2).mean((1, 2)).numpy()
        ref_l1, ref_ssim, ref_psnr = float((a - b).abs().mean()), float(LR.ssim(a, b)), float(psnr(a, b).mean())
        assert got["mse"].shape == (3,)
        assert _rel(got["mse"].cpu().numpy(), ref_mse) <= 1e-5
        assert np.abs(got["mse"].cpu().numpy() / ref_mse - 1).max() <= 1e-5
        assert abs(float(got["l1"]) - ref_l1) <= 1e-5 * ref_l1
        assert abs(float(got["ssim"]) - ref_ssim) <= 1e-5 * abs(ref_ssim)
        assert abs(float(got["psnr"]) - ref_psnr) <= 1e-4  # dB; 10 log10(1 + 1e-5) = 4.3e-5 dB with a factor of 2
        assert not any(v.requires_grad for v in got.values())
        vals.append((float(got["psnr"]), ref_psnr))
    # per-channel mean of PSNRs for (3, H, W), per-image PSNR for (1, 3, H, W): different numbers, as the reference's
    assert abs(vals[0][1] - vals[1][1]) > 1e-3
    assert abs(vals[0][0] - vals[1][0]) > 1e-3
