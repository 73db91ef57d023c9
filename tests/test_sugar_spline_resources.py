"""Register budget of the spline kernels (csrc/gsr_spline.hip): the gfx950 compile spills no VGPR to scratch (the cubic
rotation backward keeps three Log / Exp pairs and a four-term product chain live in fp64; a spill would pay a scratch
round trip per point) and keeps at least two waves per SIMD.  Device-only compile with the Makefile's flags, reading
the compiler's resource remarks only; no GPU needed."""
from kernel_budget import assert_kernel_budget, needs_hipcc

# the forward and the rows kernel are instantiated per degree
KERNELS = ("k_spline_forwardILi1E", "k_spline_forwardILi3E", "k_spline_rowsILi1E", "k_spline_rowsILi3E",
           "k_spline_knotsE")


@needs_hipcc
def test_spline_kernels_do_not_spill(tmp_path):
    assert_kernel_budget("gsr_spline.hip", tmp_path, "k_spline", dict.fromkeys(KERNELS, 2))
