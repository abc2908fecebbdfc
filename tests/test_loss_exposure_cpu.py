"""The exposure / alpha-mask additions to the loss, as far as they go without a device: the Python signatures, the
argument checks of hlgs_photo_forward / hlgs_photo_backward (which return before anything is launched) and the
errors of the Python front end."""
import ctypes as C
import inspect

import pytest
import torch

from hlgs_core import _lib as L

ERR_ARG = 1   # HLGS_ERR_ARG
CLAMP1 = 2    # HLGS_SSIM_CLAMP1
PTR = C.c_void_p(4096)  # a non-NULL pointer that is never dereferenced: every call below fails its checks first


def _err(lib):
    return lib.hlgs_last_error().decode()


def test_signatures():
    from hlgs_core import loss
    sig = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    assert sig(loss.photometric_loss) == ["image", "gt", "lambda_dssim", "invdepth", "mono_invdepth", "depth_mask",
                                          "depth_weight", "clamp_image", "exposure", "alpha_mask"]
    p = inspect.signature(loss.photometric_loss).parameters
    assert p["exposure"].default is None and p["alpha_mask"].default is None and p["clamp_image"].default is False
    assert sig(loss.image_metrics) == ["image", "gt", "alpha_mask", "clamp_image"]
    p = inspect.signature(loss.image_metrics).parameters
    assert p["alpha_mask"].default is None and p["clamp_image"].default is True


def test_photo_scratch_size_covers_both_directions():
    lib = L.load()
    tiles = -(-1920 // 128) * -(-1080 // 16)
    assert lib.hlgs_photo_scratch_size(1080, 1920) >= 4 * 12 * tiles  # 9 forward sums, 12 backward sums per tile
    assert lib.hlgs_photo_scratch_size(0, 0) > 0


def _forward(lib, H=8, W=8, image=PTR, gt=PTR, flags=0, scratch=PTR, out=PTR):
    return lib.hlgs_photo_forward(H, W, image, gt, flags, None, None, None, scratch, out, None)


def _backward(lib, H=8, W=8, image=PTR, gt=PTR, flags=0, exposure=None, dmaps=PTR, coef=PTR, grad=PTR, d_expo=None,
              scratch=PTR):
    return lib.hlgs_photo_backward(H, W, image, gt, flags, exposure, None, dmaps, coef, grad, d_expo, scratch, None)


@pytest.mark.parametrize("call", [_forward, _backward])
def test_photo_entry_points_reject_bad_arguments_before_launching(call):
    lib = L.load()
    for flags in (1, 4, CLAMP1 | 1, -1):  # HLGS_SSIM_VALID is not accepted here: only HLGS_SSIM_CLAMP1
        assert call(lib, flags=flags) == ERR_ARG
        assert "flags" in _err(lib)
    for hw in ((0, 8), (8, 0), (-1, 8)):
        assert call(lib, H=hw[0], W=hw[1]) == ERR_ARG
        assert "empty image" in _err(lib)
    required = ["image", "gt", "scratch"] + (["out"] if call is _forward else ["dmaps", "coef", "grad"])
    for name in required:
        assert call(lib, flags=CLAMP1, **{name: None}) == ERR_ARG, name
        assert "missing" in _err(lib), name


def test_exposure_gradient_needs_an_exposure():
    lib = L.load()
    assert _backward(lib, d_expo=PTR) == ERR_ARG
    assert "exposure" in _err(lib)


def test_cpu_image_raises():
    from hlgs_core.loss import image_metrics, photometric_loss
    img, gt = torch.rand(3, 16, 16), torch.rand(3, 16, 16)
    with pytest.raises(RuntimeError, match="HIP device|device tensors"):
        photometric_loss(img, gt, 0.2, exposure=torch.eye(3, 4))
    with pytest.raises(RuntimeError, match="HIP device|device tensors"):
        photometric_loss(img, gt, 0.2, alpha_mask=torch.ones(1, 16, 16))
    with pytest.raises(RuntimeError, match="HIP device|device tensors"):
        image_metrics(img, gt)


def test_shape_errors_come_first():
    from hlgs_core.loss import image_metrics, photometric_loss
    with pytest.raises(RuntimeError, match=r"\(3, H, W\)"):
        photometric_loss(torch.rand(1, 16, 16), torch.rand(1, 16, 16), 0.2, exposure=torch.eye(3, 4))
    with pytest.raises(RuntimeError, match=r"\(3, H, W\)"):
        photometric_loss(torch.rand(2, 3, 16, 16), torch.rand(2, 3, 16, 16), 0.2, alpha_mask=torch.ones(1, 16, 16))
    with pytest.raises(RuntimeError, match=r"\(3, H, W\)"):
        image_metrics(torch.rand(16, 16), torch.rand(16, 16))
    with pytest.raises(RuntimeError, match=r"\(3, 4\)"):
        photometric_loss(torch.rand(3, 16, 16), torch.rand(3, 16, 16), 0.2, exposure=torch.eye(4, 4))
    with pytest.raises(RuntimeError, match="alpha_mask must be"):
        photometric_loss(torch.rand(3, 16, 16), torch.rand(3, 16, 16), 0.2, alpha_mask=torch.ones(3, 16, 16))
