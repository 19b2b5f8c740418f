"""Register and LDS budget of the kernels in fedmx_signature.hip (CPU only:
hipcc cross-compiles for gfx950): ``incident_sig_kernel`` -- explain_rows_kernel's
standardise and forward plus 32 kept residuals and two columns' float64
accumulators per lane -- runs without scratch and without VGPR spills, two
workgroups fit a CU, and its LDS is no larger than score_rows_kernel's;
``incident_sig_fold_kernel`` has no scratch and no spills either."""
import shutil

import pytest

from fedmse_decentralized_amd.ops import build

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not build.Path("/opt/rocm/bin/hipcc").exists(),
                                reason="needs hipcc")

LDS_BYTES = 160 * 1024   # per CU on gfx950


@pytest.fixture(scope="module")
def resources():
    return build.kernel_resources("fedmx_signature.hip")


def one(res, name):
    found = {k: v for k, v in res.items() if name + "E" in k}   # (the mangled name: the name, then its argument list)
    assert len(found) == 1, list(res)
    (k, v), = found.items()
    print(k, v)
    return v


def test_signature_kernel_has_no_scratch_no_spills_and_two_workgroups_per_cu(resources):
    r = one(resources, "incident_sig_kernel")
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0, r
    assert 2 * r["lds"] <= LDS_BYTES, r
    assert r["vgpr"] + r["agpr"] <= 256, r
    assert r["occupancy"] >= 2, r


def test_signature_kernel_lds_is_no_larger_than_score_rows(resources):
    sc = [v for k, v in build.kernel_resources("fedmx_score.hip").items() if "score_rows_kernel" in k]
    assert len(sc) == 1
    assert one(resources, "incident_sig_kernel")["lds"] <= sc[0]["lds"], sc[0]


def test_fold_kernel_has_no_scratch_and_no_spills(resources):
    r = one(resources, "incident_sig_fold_kernel")
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, r
