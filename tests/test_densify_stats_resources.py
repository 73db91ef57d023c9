"""Register budget of the densification-statistics kernels (csrc/gsr_densify.hip): exactly the kernels named here, no
VGPR spill, and the occupancy stated at the kernel's attribute (device-only gfx950 compile, no GPU)."""
from kernel_budget import assert_kernel_budget, needs_hipcc

# mangled-name fragment -> waves per SIMD (amdgpu_waves_per_eu at the kernel): visible = radii > 0, visibility rows
KERNELS = {"k_dstat_viewsILb0EE": 8, "k_dstat_viewsILb1EE": 8}


@needs_hipcc
def test_densify_kernels_fit_their_budget(tmp_path):
    res = assert_kernel_budget("gsr_densify.hip", tmp_path, "k_dstat_", KERNELS, sgpr_too=True)
    assert all(r["VGPRs"] <= 64 for r in res.values()), res  # 8 waves per SIMD need at most 64
