"""Register and LDS budget of the deformation-network kernels (csrc/gsr_deform.hip): the gfx950 compile spills no VGPR
to scratch and keeps the occupancy the tile was chosen for.  k_deform_forward and k_deform_mlp are 512-thread blocks
that hold the whole MLP in LDS (111 and 129 KB of the CU's 160): one block of 8 waves per CU, 2 waves per SIMD, which
also gives each lane the 256 registers the backward's 55 fp64 accumulators need.  The texel kernels hold no LDS and are
bound by registers (5 waves per SIMD); the reduction is trivial (8).  Device-only compile with the Makefile's flags,
reading the compiler's resource remarks only; no GPU needed."""
import os
import shutil

import pytest

from test_kernel_resources import HIPCC, kernel_resources

# kernel -> least occupancy [waves / SIMD], the compiler's figure for the chosen tile
KERNELS = {"k_deform_forwardE": 2, "k_deform_mlpE": 2, "k_deform_reduceE": 8, "k_deform_spatialE": 5,
           "k_deform_timeE": 5}


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not in this image")
def test_deform_kernels_do_not_spill(tmp_path):
    res = {k: v for k, v in kernel_resources("gsr_deform.hip", tmp_path).items() if "k_deform" in k}
    assert len(res) == len(KERNELS), sorted(res)
    for name, occupancy in KERNELS.items():
        found = [r for k, r in res.items() if name in k]
        assert len(found) == 1, name
        assert found[0].get("VGPRs Spill", 0) == 0, (name, found[0])
        assert found[0].get("Occupancy [waves/SIMD]", 0) >= occupancy, (name, found[0])
