"""Scenes that reach three branches hlgs_core.synthetic.make_gaussians never does (tests/test_clamp_scenes_cpu.py
asserts from the oracle that they do, for every size the GPU tests use; tests/test_gpu_clamps.py and the float64
cases of tests/test_oracle.py run on them):

* the frustum clamp of the EWA Jacobian: t.x / t.z and t.y / t.z limited to +-1.3 tanfov (forward.cu:141-176), with
  the backward's dL/dt.x, dL/dt.y zeroed there (backward.cu:185-186, 310-312) -- contributing Gaussians whose centres
  lie outside 1.3x the frustum;
* the SH colour clamp at 0 (forward.cu computeColorFromSH, backward.cu:23-142) -- about a third of the channels;
* the anti-aliasing floor h = sqrt(max(2.5e-5, det / det_h)) (backward.cu:212-246) -- splats far below a pixel.

Quaternions of a scene can be left unnormalised: computeCov3D uses them as given (forward.cu:181-215)."""
import numpy as np

from hlgs_core import synthetic as S

# (P, W, H, seed) of every frustum / AA-floor scene the GPU tests build; 100 x 75 and 90 x 70 are no multiples of 16
FRUSTUM_SIZES = ((300, 64, 48, 1), (1200, 100, 75, 2), (2000, 128, 96, 3), (3000, 128, 96, 4))
AA_SIZES = ((300, 64, 48, 1), (1500, 90, 70, 2), (3000, 128, 96, 3))
REALCAM = 5  # the rotated camera of the reference's dataset the clamp tests use (tests/golden/golden_realcam.npz)


def camera_space(means, cam):
    """World-space centres in the camera's frame, float64 (the inverse of make_gaussians' placement)."""
    Rc2w, T = np.asarray(cam.get("R", np.eye(3)), np.float64), np.asarray(cam.get("T", np.zeros(3)), np.float64)
    return (np.asarray(means, np.float64) + Rc2w @ T) @ Rc2w


def clamp_classes(sc, cam):
    """-> (xc, yc): per Gaussian, whether |t.x / t.z| > 1.3 tanfovx and |t.y / t.z| > 1.3 tanfovy with t the
    view-space centre (float64, through the view matrix the rasterizer gets)."""
    view = cam["viewmatrix"].numpy().astype(np.float64).reshape(4, 4)
    t = np.c_[sc["means3D"].astype(np.float64), np.ones(len(sc["means3D"]))] @ view
    return np.abs(t[:, 0] / t[:, 2]) > 1.3 * cam["tanfovx"], np.abs(t[:, 1] / t[:, 2]) > 1.3 * cam["tanfovy"]


def unnormalise_quaternions(sc, seed):
    """Scale every quaternion by U(0.7, 1.4), in place; returns sc."""
    rng = np.random.Generator(np.random.PCG64(seed + 4000))
    k = rng.uniform(0.7, 1.4, (sc["rotations"].shape[0], 1))
    sc["rotations"] = np.ascontiguousarray((sc["rotations"] * k).astype(np.float32))
    return sc


def frustum_clamp_scene(P, deg, W, H, seed, cam=None, unnormalised=False):
    """-> (scene, cam): wide splats (sigma 5-14 px at W = 64, growing with W so that the same share of the off-frame
    centres still reaches the frame; depth 3-12) whose centres are re-placed in camera space so that
    rows [0, P/2) have |x/z| in (1.32, 1.9) tanfovx and rows [P/4, 3P/4) have |y/z| in (1.32, 1.9) tanfovy (random
    signs), every other coordinate within 1.25 tanfov: the four classes x-clamped, both, y-clamped, neither, a quarter
    of the rows each.  The DC coefficients are N(-1.2, 1.2), so about a third of the colour channels clamp at 0.
    cam: a camera of another pose (default S.make_camera(W, H)); the centres go through its R, T as make_gaussians'
    do.  unnormalised: see unnormalise_quaternions."""
    cam = cam or S.make_camera(W, H)
    sc = S.make_gaussians(P, deg, cam, seed, zmin=3, zmax=12, sigma_px=(5.0 * W / 64, 14.0 * W / 64))
    rng = np.random.Generator(np.random.PCG64(seed + 3000))
    z = camera_space(sc["means3D"], cam)[:, 2]
    fx_ = rng.uniform(0.0, 1.25, P)
    fy_ = rng.uniform(0.0, 1.25, P)
    fx_[: P // 2] = rng.uniform(1.32, 1.9, P // 2)
    fy_[P // 4: 3 * P // 4] = rng.uniform(1.32, 1.9, 3 * P // 4 - P // 4)
    x = fx_ * rng.choice([-1.0, 1.0], P) * cam["tanfovx"] * z
    y = fy_ * rng.choice([-1.0, 1.0], P) * cam["tanfovy"] * z
    Rc2w, T = np.asarray(cam["R"], np.float64), np.asarray(cam["T"], np.float64)
    sc["means3D"] = np.ascontiguousarray((np.stack([x, y, z], 1) @ Rc2w.T - Rc2w @ T).astype(np.float32))
    sc["shs"][:, 0, :] = rng.normal(-1.2, 1.2, (P, 3)).astype(np.float32)
    if unnormalised:
        unnormalise_quaternions(sc, seed)
    return sc, cam


def aa_floor_scene(P, W, H, seed, deg=1):
    """-> (scene, cam): near-isotropic splats (axes within +-10 %) at depth 4-8, each centred within 0.05 px of its own
    pixel's centre.  Rows [0, P/2) have sigma in [0.005, 0.03] px: det / det_h <= 2.5e-5, the anti-aliasing factor sits
    on its floor 0.005 and its gradient is cut.  The other rows have sigma in [0.05, 0.3] px, above the floor.
    Opacities are 0.85-0.99, so a floor row still reaches alpha = 0.005 o >= 1 / 255 at its pixel."""
    cam = S.make_camera(W, H)
    sc = S.make_gaussians(P, deg, cam, seed, zmin=4, zmax=8)
    rng = np.random.Generator(np.random.PCG64(seed + 5000))
    z = sc["means3D"][:, 2].astype(np.float64)
    pixel = rng.choice(W * H, P, replace=False)
    px = pixel % W + rng.uniform(-0.05, 0.05, P)
    py = pixel // W + rng.uniform(-0.05, 0.05, P)
    sc["means3D"][:, 0] = (((2 * px + 1) / W - 1) * cam["tanfovx"] * z).astype(np.float32)
    sc["means3D"][:, 1] = (((2 * py + 1) / H - 1) * cam["tanfovy"] * z).astype(np.float32)
    sigma = np.concatenate([rng.uniform(0.005, 0.03, P // 2), rng.uniform(0.05, 0.3, P - P // 2)])
    sc["scales"] = np.ascontiguousarray(((sigma * z / cam["fx"])[:, None] * rng.uniform(0.9, 1.1, (P, 3)))
                                        .astype(np.float32))
    sc["opacities"] = rng.uniform(0.85, 0.99, (P, 1)).astype(np.float32)
    return sc, cam


def two_view_cameras(W, H):
    """The two cameras of tests/test_gpu_dp.py's colour-factored exchange cases."""
    return [S.make_camera(W, H), S.make_camera(W, H, T=np.array([0.3, -0.1, 0.2]))]


def two_view_scene(kind, W=160, H=96):
    """-> (scene, cams) of a colour-factored exchange case, 16 SH rows: "plain" is make_gaussians(6000) as those cases
    always had it (a channel clamps about 2e-4 of the time), "frustum" the frustum-clamp scene placed for the first
    camera, where a third of the channels clamp."""
    cams = two_view_cameras(W, H)
    if kind == "plain":
        return S.make_gaussians(6000, 3, cams[0], seed=7), cams
    assert kind == "frustum"
    return frustum_clamp_scene(3000, 3, W, H, seed=7, cam=cams[0])[0], cams


def clamp_bits_of_two_views(sc, cams, D):
    """-> (a, b, seen): the oracle's clamp bitmasks (bit c = channel c clamped at 0) of the scene at active degree D
    under the two cameras, and the rows visible (radius > 0) in both."""
    from oracle import oracle as O
    frs = [O.forward(dict(sc, sh_degree=D), S.cam_numpy(c)) for c in cams]
    return frs[0].clamped, frs[1].clamped, (frs[0].radii > 0) & (frs[1].radii > 0)


def alt_layout(sc, antialiasing=True):
    """The same Gaussians in the alt rasterizer's layout: dc (P, 1, 3) + the remaining coefficients."""
    out = dict(sc)
    out["dc"] = np.ascontiguousarray(sc["shs"][:, :1])
    out["shs"] = np.ascontiguousarray(sc["shs"][:, 1:])
    out["alt"] = True
    out["antialiasing"] = antialiasing
    return out
