"""Register budget of the dynamic-SuGaR kernels (csrc/gsr_dynamic.hip): the gfx950 compile spills no VGPR to scratch
(their fp64 chains would pay a scratch round trip per item).  Device-only compile with the Makefile's flags, reading
the compiler's resource remarks only; no GPU needed."""
from kernel_budget import assert_kernel_budget, needs_hipcc

KERNELS = ("k_skin_nodes", "k_skin_forward", "k_skin_vertex", "k_skin_verts_sum", "k_skin_node", "k_timed_forward",
           "k_timed_face", "k_timed_vertex", "k_timed_gauss")


@needs_hipcc
def test_dynamic_kernels_do_not_spill(tmp_path):
    assert_kernel_budget("gsr_dynamic.hip", tmp_path, ("k_skin", "k_timed"), dict.fromkeys(KERNELS, 2))
