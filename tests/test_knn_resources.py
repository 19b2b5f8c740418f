"""Register and LDS budget of ``knn_score_kernel`` (fedmx_knn.hip; CPU only:
hipcc cross-compiles for gfx950): every instantiation (k = 1 .. 16 neighbours
in a sorted register list) runs without scratch and without VGPR spills, and
its train tile leaves room for a second workgroup on the CU."""
import shutil

import pytest

from fedmse_decentralized_amd.ops import build

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not build.Path("/opt/rocm/bin/hipcc").exists(),
                                reason="needs hipcc")

LDS_BYTES = 160 * 1024   # per CU on gfx950


def test_knn_kernels_have_no_scratch_and_no_spills():
    res = build.kernel_resources("fedmx_knn.hip")
    kernels = {k: v for k, v in res.items() if "knn_score_kernel" in k}
    assert len(kernels) == 16, list(res)
    for name, r in kernels.items():
        print(name, r)
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (name, r)
        assert r["lds"] <= LDS_BYTES, (name, r)
        # __launch_bounds__(256, 2): a workgroup is one wave per SIMD, and the
        # kernel is meant to run two workgroups per CU (two waves per SIMD, the
        # second hiding the first's LDS latency under float64 VALU work).  Two
        # workgroups must fit the LDS, and two waves share a SIMD's 512
        # registers per lane: 256 each.
        assert 2 * r["lds"] <= LDS_BYTES, (name, r)
        assert r["vgpr"] + r["agpr"] <= 256, (name, r)
        assert r["occupancy"] >= 2, (name, r)
