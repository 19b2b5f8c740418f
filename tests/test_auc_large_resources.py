"""Register budget of the multi-workgroup AUC kernels (fedmx_auc_large.hip;
CPU only: hipcc cross-compiles for gfx950): no scratch and no spills in any
of the four, and the 1024-thread pairs kernel within 64 VGPRs."""
import shutil

import pytest

from fedmse_decentralized_amd.ops import build

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not build.Path("/opt/rocm/bin/hipcc").exists(),
                                reason="needs hipcc")

KERNELS = ("auc_large_count_kernel", "auc_large_partition_kernel", "auc_large_pairs_kernel",
           "auc_large_finalize_kernel")


@pytest.fixture(scope="module")
def resources():
    return build.kernel_resources("fedmx_auc_large.hip")


def test_auc_large_kernels_have_no_scratch_and_no_spills(resources):
    for name in KERNELS:
        hits = {k: v for k, v in resources.items() if name in k}
        assert len(hits) == 1, (name, list(resources))
        (r,) = hits.values()
        print(name, r)
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)


def test_pairs_kernel_fits_1024_threads(resources):
    (r,) = [v for k, v in resources.items() if "auc_large_pairs_kernel" in k]
    assert r["vgpr"] <= 64, r   # 1024 threads: 16 waves, 4 per SIMD
    assert r["lds"] == 0, r     # the chunk and the two sums live in the dynamic region only
