"""The compiler's resource remarks for a kernel source (device-only gfx950 compile, the Makefile's flags, no GPU), and
the budget the kernel tests hold them to.  No tests here."""
import os
import re
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "threestudio-3dgs_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
needs_hipcc = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not in this image")


def kernel_resources(src, tmp_path):
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-slp-vectorize", "--cuda-device-only",
           "-c", src, "-o", str(tmp_path / "k.o"), "-Rpass-analysis=kernel-resource-usage"]
    res = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    out, name = {}, None
    for line in res.stderr.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs Spill|SGPRs Spill|VGPRs|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and name is not None:
            out[name][m.group(1)] = int(m.group(2))
    return out


def assert_kernel_budget(src, tmp_path, prefix, kernels, sgpr_too=False):
    """The kernels of `src` whose mangled name holds `prefix` (or one of several) are exactly those of `kernels`, one
    each; none spills a VGPR to scratch (nor an SGPR, with sgpr_too) and each keeps the least occupancy [waves / SIMD]
    that `kernels` maps it to.  A name that ends in the mangling's "E" is looked for as it is; a bare name must be
    followed by "E" or "N", so that k_skin_node is not found in k_skin_nodes.  Returns the remarks by mangled name."""
    prefixes = (prefix,) if isinstance(prefix, str) else prefix
    res = {k: v for k, v in kernel_resources(src, tmp_path).items() if any(p in k for p in prefixes)}
    assert len(res) == len(kernels), sorted(res)
    for name, occupancy in kernels.items():
        found = [r for k, r in res.items() if (name in k if name.endswith("E") else name + "E" in k or name + "N" in k)]
        assert len(found) == 1, (name, sorted(res))
        assert found[0].get("Occupancy [waves/SIMD]", 0) >= occupancy, (name, found[0])
    for name, r in res.items():
        assert r.get("VGPRs Spill", 0) == 0 and not (sgpr_too and r.get("SGPRs Spill", 0)), (name, r)
    return res
