"""Register and LDS budget of ``explain_rows_kernel`` (fedmx_explain.hip; CPU
only: hipcc cross-compiles for gfx950): the kernel -- score_rows_kernel's
paths plus 32 kept residuals and 32 ranking keys per lane -- runs without
scratch (no dynamically indexed register array) and without VGPR spills, and
its LDS leaves room for a second workgroup on the CU."""
import shutil

import pytest

from fedmse_decentralized_amd.ops import build

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not build.Path("/opt/rocm/bin/hipcc").exists(),
                                reason="needs hipcc")

LDS_BYTES = 160 * 1024   # per CU on gfx950


def test_explain_kernel_has_no_scratch_no_spills_and_two_workgroups_per_cu():
    res = build.kernel_resources("fedmx_explain.hip")
    kernels = {k: v for k, v in res.items() if "explain_rows_kernel" in k}
    assert len(kernels) == 1, list(res)
    for name, r in kernels.items():
        print(name, r)
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (name, r)
        assert 2 * r["lds"] <= LDS_BYTES, (name, r)
        assert r["vgpr"] + r["agpr"] <= 256, (name, r)
        assert r["occupancy"] >= 2, (name, r)


def test_explain_kernel_lds_is_no_larger_than_score_rows():
    ex = [v for k, v in build.kernel_resources("fedmx_explain.hip").items() if "explain_rows_kernel" in k]
    sc = [v for k, v in build.kernel_resources("fedmx_score.hip").items() if "score_rows_kernel" in k]
    assert len(ex) == 1 and len(sc) == 1
    assert ex[0]["lds"] <= sc[0]["lds"], (ex[0], sc[0])
