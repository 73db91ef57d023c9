"""Register budget of the spline kernels (csrc/gsr_spline.hip): the gfx950 compile spills no VGPR to scratch (the cubic
rotation backward keeps three Log / Exp pairs and a four-term product chain live in fp64; a spill would pay a scratch
round trip per point) and keeps at least two waves per SIMD.  Device-only compile with the Makefile's flags, reading
the compiler's resource remarks only; no GPU needed."""
import os
import shutil

import pytest

from test_kernel_resources import HIPCC, kernel_resources

# the forward and the rows kernel are instantiated per degree
KERNELS = ("k_spline_forwardILi1E", "k_spline_forwardILi3E", "k_spline_rowsILi1E", "k_spline_rowsILi3E",
           "k_spline_knotsE")


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not in this image")
def test_spline_kernels_do_not_spill(tmp_path):
    res = {k: v for k, v in kernel_resources("gsr_spline.hip", tmp_path).items() if "k_spline" in k}
    assert len(res) == len(KERNELS), sorted(res)
    for name in KERNELS:
        assert any(name in k for k in res), name
    for name, r in res.items():
        assert r.get("VGPRs Spill", 0) == 0, (name, r)
        assert r.get("Occupancy [waves/SIMD]", 0) >= 2, (name, r)
