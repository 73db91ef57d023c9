"""Register budget of the dynamic-SuGaR kernels (csrc/gsr_dynamic.hip): the gfx950 compile spills no VGPR to scratch
(their fp64 chains would pay a scratch round trip per item).  Device-only compile with the Makefile's flags, reading
the compiler's resource remarks only; no GPU needed."""
import os
import shutil

import pytest

from test_kernel_resources import HIPCC, kernel_resources

KERNELS = ("k_skin_nodes", "k_skin_forward", "k_skin_vertex", "k_skin_verts_sum", "k_skin_node", "k_timed_forward",
           "k_timed_face", "k_timed_vertex", "k_timed_gauss")


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not in this image")
def test_dynamic_kernels_do_not_spill(tmp_path):
    res = {k: v for k, v in kernel_resources("gsr_dynamic.hip", tmp_path).items() if "k_skin" in k or "k_timed" in k}
    assert len(res) == len(KERNELS), sorted(res)
    for name in KERNELS:
        assert any(name + "E" in k or name + "N" in k for k in res), name
    for name, r in res.items():
        assert r.get("VGPRs Spill", 0) == 0, (name, r)
        assert r.get("Occupancy [waves/SIMD]", 0) >= 2, (name, r)
