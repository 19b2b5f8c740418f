"""Register and LDS budget of ``monitor_rows_kernel`` (fedmx_monitor.hip; CPU
only: hipcc cross-compiles for gfx950), from the compiled code object's
metadata: the kernel -- score_rows_kernel's paths plus two columns' float64 and
integer accumulators per lane, the score edges and a histogram in LDS -- keeps
its static LDS at or under 81,920 B, so two workgroups share a CU's 160 KB, and
runs without scratch and without VGPR spills."""
import shutil

import pytest

from fedmse_decentralized_amd.ops import build

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not build.Path("/opt/rocm/bin/hipcc").exists(),
                                reason="needs hipcc")

LDS_LIMIT = 81920   # half of a gfx950 CU's 160 KB


def test_monitor_kernel_has_no_scratch_no_spills_and_two_workgroups_per_cu():
    res = build.kernel_resources("fedmx_monitor.hip")
    kernels = {k: v for k, v in res.items() if "monitor_rows_kernel" in k}
    assert len(kernels) == 1, list(res)
    for name, r in kernels.items():
        print(name, r)
        assert r["lds"] <= LDS_LIMIT, (name, r)
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (name, r)
        assert r["vgpr"] + r["agpr"] <= 256 and r["occupancy"] >= 2, (name, r)
    fold = [v for k, v in res.items() if "monitor_fold_kernel" in k]
    assert len(fold) == 1 and fold[0]["scratch"] == 0 and fold[0]["vgpr_spill"] == 0 and fold[0]["lds"] <= 65536, fold
