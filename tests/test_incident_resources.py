"""Register and LDS budget of the incident kernels (fedmx_incident.hip; CPU
only: hipcc cross-compiles for gfx950), from the compiled code object's
metadata: every kernel runs without scratch and without VGPR spills and keeps
its static LDS at or under 65,536 B."""
import shutil

import pytest

from fedmse_decentralized_amd.ops import build

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not build.Path("/opt/rocm/bin/hipcc").exists(),
                                reason="needs hipcc")

LDS_LIMIT = 65536


def test_incident_kernels_have_no_scratch_no_spills_and_bounded_lds():
    res = build.kernel_resources("fedmx_incident.hip")
    names = sorted(res)
    for part in ("incident_kernelILi0E", "incident_kernelILi1E", "incident_kernelILi2E", "incident_scan_kernel",
                 "incident_finish_kernel"):
        assert sum(part in k for k in names) == 1, (part, names)
    assert len(names) == 5, names
    for name, r in res.items():
        print(name, r)
        assert r["scratch"] == 0 and r["vgpr_spill"] == 0, (name, r)
        assert r["lds"] <= LDS_LIMIT, (name, r)
