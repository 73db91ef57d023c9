"""Register budget of the ARAP kernels (csrc/gsr_arap.hip): the gfx950 compile spills no VGPR to scratch (their fp64
row sums would pay a scratch round trip per edge) and keeps at least 2 waves per SIMD.  Device-only compile with the
Makefile's flags, reading the compiler's resource remarks only; no GPU needed."""
from kernel_budget import assert_kernel_budget, needs_hipcc

KERNELS = ("k_arap_forward", "k_arap_reduce", "k_arap_backward")


@needs_hipcc
def test_arap_kernels_do_not_spill(tmp_path):
    assert_kernel_budget("gsr_arap.hip", tmp_path, "k_arap", dict.fromkeys(KERNELS, 2))
