"""Register and LDS budget of the deformation-network kernels (csrc/gsr_deform.hip): the gfx950 compile spills no VGPR
to scratch and keeps the occupancy the tile was chosen for.  k_deform_forward and k_deform_mlp are 512-thread blocks
that hold the whole MLP in LDS (111 and 129 KB of the CU's 160): one block of 8 waves per CU, 2 waves per SIMD, which
also gives each lane the 256 registers the backward's 55 fp64 accumulators need.  The texel kernels hold no LDS and are
bound by registers (5 waves per SIMD); the reduction is trivial (8).  Device-only compile with the Makefile's flags,
reading the compiler's resource remarks only; no GPU needed."""
from kernel_budget import assert_kernel_budget, needs_hipcc

# kernel -> least occupancy [waves / SIMD], the compiler's figure for the chosen tile
KERNELS = {"k_deform_forwardE": 2, "k_deform_mlpE": 2, "k_deform_reduceE": 8, "k_deform_spatialE": 5,
           "k_deform_timeE": 5}


@needs_hipcc
def test_deform_kernels_do_not_spill(tmp_path):
    assert_kernel_budget("gsr_deform.hip", tmp_path, "k_deform", KERNELS)
