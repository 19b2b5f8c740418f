"""Register budget of ``detect_kernel`` (fedmx_detect.hip; CPU only: hipcc
cross-compiles for gfx950): no scratch and no spills, so the radix select's
eight passes and the counting pass run from registers and 2 KiB of LDS."""
import shutil

import pytest

from fedmse_decentralized_amd.ops import build

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not build.Path("/opt/rocm/bin/hipcc").exists(),
                                reason="needs hipcc")


def test_detect_kernel_has_no_scratch_and_no_spills():
    res = build.kernel_resources("fedmx_detect.hip")
    kernels = {k: v for k, v in res.items() if "detect_kernel" in k}
    assert len(kernels) == 1, list(res)
    (r,) = kernels.values()
    print(r)
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, r
    assert r["vgpr"] <= 64 and r["lds"] <= 4096, r   # 1024 threads: 16 waves, at most 128 VGPRs each
