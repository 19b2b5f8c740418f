"""Register and LDS budget of ``geomed_step_kernel`` (fedmx_geomed.hip; CPU
only: hipcc cross-compiles for gfx950): no scratch, no VGPR or SGPR spills, and
at most 32 KB of LDS (the row table, the weights and the fold buffers at k =
1024)."""
import shutil

import pytest

from fedmse_decentralized_amd.ops import build

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not build.Path("/opt/rocm/bin/hipcc").exists(),
                                reason="needs hipcc")


@pytest.fixture(scope="module")
def resources():
    return build.kernel_resources("fedmx_geomed.hip")


def test_geomed_kernel_is_the_only_kernel(resources):
    assert len(resources) == 1 and "geomed_step_kernelE" in next(iter(resources)), list(resources)


def test_geomed_kernel_has_no_scratch_no_spills_and_fits_its_lds_budget(resources):
    (name, r), = resources.items()
    print(name, r)
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, r
    assert r["lds"] <= 32 * 1024, r
    assert r["vgpr"] + r["agpr"] <= 128, r   # (at least four waves per SIMD)
