"""bench.py's launch contract on the CPU (no GPU work): `--gpus N` means N ranks.

`python bench.py --gpus 2` with no launcher starts torch.distributed.run with two ranks as a child process, and the
rank-0 line says n_gpus 2; `--gpus N` that disagrees with an existing WORLD_SIZE is an error, not a world-1 line.
`--dry-run` stops each rank after the process group has formed (gloo here), so no GPU is needed.
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _env(**kw):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR",
                                                              "MASTER_PORT")}
    env.update(HLGS_DIST_BACKEND="gloo", OMP_NUM_THREADS="1", **kw)
    return env


def _line(out):
    lines = [ln for ln in out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out
    return json.loads(lines[0])


def test_gpus_2_without_launcher_starts_two_ranks():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--dry-run"], env=_env(), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    line = _line(r.stdout)
    assert line["n_gpus"] == 2 and line["ranks_joined"] == 2 and line["gpus_arg"] == 2


def test_gpus_1_default_is_one_rank():
    r = subprocess.run([sys.executable, BENCH, "--dry-run"], env=_env(), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert _line(r.stdout)["n_gpus"] == 1


def test_gpus_disagreeing_with_world_size_fails():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "8", "--dry-run"], env=_env(WORLD_SIZE="1"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "WORLD_SIZE=1" in r.stderr
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]


def test_full_and_dump_outputs_are_options():
    r = subprocess.run([sys.executable, BENCH, "--full", "--dump-outputs", "unused", "--dry-run"], env=_env(),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert _line(r.stdout)["n_gpus"] == 1


def test_steps_zero_rejected():
    r = subprocess.run([sys.executable, BENCH, "--steps", "0", "--dry-run"], env=_env(), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode != 0
    assert "--steps" in r.stderr


def test_dump_outputs_sample_is_seeded_and_bounded(tmp_path, monkeypatch):
    """dump_outputs on host tensors: arrays under the caps are written whole, larger ones as the same seeded sample
    of pixels / rows on every call, float32 (the index arrays float64)."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(bench, "DUMP_MAX_PIXELS", 100)
    monkeypatch.setattr(bench, "DUMP_MAX_ROWS", 50)
    g = torch.Generator().manual_seed(0)
    P, H, W = 70, 12, 10

    def param(*shape):
        p = torch.zeros(*shape, requires_grad=True)
        p.grad = torch.randn(*shape, generator=g)
        return p
    params = [param(P, 3), param(P, 3), param(P, 4), param(P, 1), param(P, 16, 3)]
    st = dict(params=params, means2D=param(P, 3), color=torch.randn(3, H, W, generator=g),
              invd=torch.randn(1, H, W, generator=g))
    radii = torch.arange(P, dtype=torch.int32)
    bench.dump_outputs(str(tmp_path / "a"), st, radii)
    bench.dump_outputs(str(tmp_path / "b"), st, radii)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(k + ".npy" for k in ("color", "invdepth", "radii", "dmean3D", "dmean2D", "dopacity",
                                                "dscale", "drot", "dsh", "sample_pixels", "sample_rows"))
    a = {n[:-4]: np.load(tmp_path / "a" / n) for n in names}
    for n in names:
        np.testing.assert_array_equal(a[n[:-4]], np.load(tmp_path / "b" / n))
        assert a[n[:-4]].dtype == (np.float64 if n.startswith("sample_") else np.float32)
    rows, pix = a["sample_rows"].astype(int), a["sample_pixels"].astype(int)
    assert len(rows) == 50 and len(np.unique(rows)) == 50 and len(pix) == 100 and len(np.unique(pix)) == 100
    np.testing.assert_array_equal(a["radii"], rows.astype(np.float32))
    np.testing.assert_array_equal(a["dsh"], params[4].grad.numpy()[rows])
    np.testing.assert_array_equal(a["color"], st["color"].numpy().reshape(3, -1)[:, pix])
    # under the caps: written whole, no index arrays
    monkeypatch.setattr(bench, "DUMP_MAX_PIXELS", H * W)
    monkeypatch.setattr(bench, "DUMP_MAX_ROWS", P)
    bench.dump_outputs(str(tmp_path / "c"), st, radii)
    assert "sample_rows.npy" not in os.listdir(tmp_path / "c")
    np.testing.assert_array_equal(np.load(tmp_path / "c" / "dmean3D.npy"), params[0].grad.numpy())
    assert np.load(tmp_path / "c" / "invdepth.npy").shape == (1, H, W)


def test_gpus_zero_rejected():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "0", "--dry-run"], env=_env(), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode != 0
