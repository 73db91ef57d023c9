"""Register budget of the mesh-regulariser kernels (csrc/gsr_meshreg.hip): the gfx950 compile spills no VGPR to scratch
(their fp64 row sums would pay a scratch round trip per entry) and keeps at least 2 waves per SIMD.  Device-only
compile with the Makefile's flags, reading the compiler's resource remarks only; no GPU needed."""
from kernel_budget import assert_kernel_budget, needs_hipcc

KERNELS = ("k_nc_forward", "k_nc_corner_rows", "k_nc_gather", "k_lap_forward", "k_lap_rows", "k_lap_gather",
           "k_meshreg_reduce")


@needs_hipcc
def test_meshreg_kernels_do_not_spill(tmp_path):
    res = assert_kernel_budget("gsr_meshreg.hip", tmp_path, ("k_nc_", "k_lap_", "k_meshreg_"),
                               dict.fromkeys(KERNELS, 2))
    for name, r in sorted(res.items()):
        print(name, r)
