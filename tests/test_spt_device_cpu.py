"""CPU-side checks of the device SPT build's boundary (csrc/spt_build.hip): the C ABI is declared, exported and bound,
its scratch query is sane, the Python entry point refuses to run without a HIP device, and densify_round has the
switch, off by default.  The build itself is checked on the GPU in tests/test_gpu_spt_build.py."""
import inspect

import pytest
import torch

from hlgs_core import _lib as L

NEW = ("hlgs_spt_device_scratch_size", "hlgs_spt_build_device", "hlgs_spt_emit_device")


def test_device_build_is_declared_exported_and_bound():
    lib = L.load()
    declared = L.header_functions()
    for name in NEW:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in L._SIGS, name
    sizes = [lib.hlgs_spt_device_scratch_size(G) for G in (1, 1000, 2_000_000)]
    assert sizes[0] > 0
    assert sizes[0] <= sizes[1] <= sizes[2]
    assert sizes[2] >= 2_000_000 * 4 * 20  # the packed rows, the entries and the sort's double buffers at least


def test_device_build_needs_a_hip_device():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from hlgs_core import spt
    nodes = torch.zeros((1, 6), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="HIP device"):
        spt.build_hierarchical_spt_device(nodes, torch.zeros(1, 3), torch.zeros(1, 3), 0, 1.0, 0.02)


def test_densify_round_has_the_switch_off_by_default():
    from hlgs_core import mcmc
    p = inspect.signature(mcmc.densify_round).parameters["spt_on_device"]
    assert p.kind == inspect.Parameter.KEYWORD_ONLY and p.default is False
