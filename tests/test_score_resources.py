"""Register and LDS budget of ``score_rows_kernel`` (fedmx_score.hip; CPU
only: hipcc cross-compiles for gfx950): the kernel -- one function holding the
compact / identity forward order times float64 / float32 input times standard
/ minmax scaler paths -- runs without scratch and without VGPR spills, and its
weights, four wave tiles and latent scratch leave room for a second workgroup
on the CU."""
import shutil

import pytest

from fedmse_decentralized_amd.ops import build

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not build.Path("/opt/rocm/bin/hipcc").exists(),
                                reason="needs hipcc")

LDS_BYTES = 160 * 1024   # per CU on gfx950


def test_score_kernel_has_no_scratch_no_spills_and_two_workgroups_per_cu():
    res = build.kernel_resources("fedmx_score.hip")
    kernels = {k: v for k, v in res.items() if "score_rows_kernel" in k}
    assert len(kernels) == 1, list(res)
    for name, r in kernels.items():
        print(name, r)
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (name, r)
        # __launch_bounds__(256, 2): two workgroups per CU, two waves per SIMD,
        # each with half of the SIMD's 512 registers per lane
        assert 2 * r["lds"] <= LDS_BYTES, (name, r)
        assert r["vgpr"] + r["agpr"] <= 256, (name, r)
        assert r["occupancy"] >= 2, (name, r)
