"""Register budget of the timed view set's per-Gaussian backward (csrc/gsr_timed.hip): exactly the kernels named here,
no VGPR spill, and the occupancy floor stated at each kernel's attribute (device-only gfx950 compile, no GPU)."""
from kernel_budget import assert_kernel_budget, needs_hipcc

# mangled-name fragment -> waves per SIMD (amdgpu_waves_per_eu at the kernel): one and two colours
KERNELS = {"k_tv_gradILb0EE": 3, "k_tv_gradILb1EE": 3}


@needs_hipcc
def test_timed_kernels_fit_their_budget(tmp_path):
    assert_kernel_budget("gsr_timed.hip", tmp_path, "k_tv_", KERNELS)


@needs_hipcc
def test_timed_preprocess_keeps_the_shared_kernel_occupancy(tmp_path):
    """k_preprocess_timed shares the body of k_preprocess: no spill, the same 6 waves per SIMD; and the shared kernels
    keep theirs."""
    assert_kernel_budget("gsr_preprocess.hip", tmp_path, "k_preprocess",
                         {"k_preprocess_timedE": 6, "k_preprocessILb0EE": 6, "k_preprocessILb1EE": 6})
