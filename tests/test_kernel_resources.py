"""Register budget of the hot kernels: the gfx950 compile of the blend and per-Gaussian backward sources
has no VGPR spills to scratch beyond the two measured, documented trade-offs below (a spill in
the backward blend's replay loop would cost a scratch round trip per pair).  Device-only
compile with the Makefile's flags, no GPU needed.  SGPR spills are not checked: they land in VGPR
lanes (v_writelane / v_readlane), not in scratch memory."""
import pytest

from kernel_budget import kernel_resources, needs_hipcc

# mangled-name fragment -> VGPRs allowed to spill, each an occupancy choice measured on the GPU and
# stated at the kernel's attribute: the two-colour per-Gaussian backward at 4 waves per SIMD spills outside the
# row loop (gsr_backward.hip, C5 only); the per-Gaussian backward with SH at 3 waves per SIMD spills 7 VGPRs,
# stored before and reloaded after its view loop (profiles/r04/gauss_accum_ab.txt).  The one-colour tile-wave
# forward (6 waves per SIMD) and the lockstep backward (5 waves per SIMD) spill nothing since round 6 (their
# loop-invariant per-lane addresses and uniform constants are formed where used or kept in scalar registers): a
# spill reload inside their loops would also wait for every memory operation in flight.
ALLOWED_VGPR_SPILL = {"17k_render_fwd_tileILb0E": 0, "11k_view_gradILb1E": 4, "12k_render_bwdE": 0,
                      "13k_gauss_accum": 7}


@needs_hipcc
@pytest.mark.parametrize("src", ["gsr_render.hip", "gsr_backward.hip"])
def test_hot_kernels_do_not_spill(src, tmp_path):
    res = kernel_resources(src, tmp_path)
    kernels = {k: v for k, v in res.items() if "k_render" in k or "k_view_grad" in k or "k_gauss_accum" in k}
    assert kernels, "no hot kernels found in " + src
    for name, r in kernels.items():
        allowed = max([n for frag, n in ALLOWED_VGPR_SPILL.items() if frag in name] or [0])
        assert r.get("VGPRs Spill", 0) <= allowed, (name, r)
        assert r.get("Occupancy [waves/SIMD]", 0) >= 2, (name, r)
