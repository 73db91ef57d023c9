"""Register budget of the ARAP kernels (csrc/gsr_arap.hip): the gfx950 compile spills no VGPR to scratch (their fp64
row sums would pay a scratch round trip per edge) and keeps at least 2 waves per SIMD.  Device-only compile with the
Makefile's flags, reading the compiler's resource remarks only; no GPU needed."""
import os
import shutil

import pytest

from test_kernel_resources import HIPCC, kernel_resources

KERNELS = ("k_arap_forward", "k_arap_reduce", "k_arap_backward")


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not in this image")
def test_arap_kernels_do_not_spill(tmp_path):
    res = {k: v for k, v in kernel_resources("gsr_arap.hip", tmp_path).items() if "k_arap" in k}
    assert len(res) == len(KERNELS), sorted(res)
    for name in KERNELS:
        assert any(name + "E" in k or name + "N" in k for k in res), name
    for name, r in res.items():
        assert r.get("VGPRs Spill", 0) == 0, (name, r)
        assert r.get("Occupancy [waves/SIMD]", 0) >= 2, (name, r)
