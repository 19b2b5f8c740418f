import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# the reference's device lists and, packed, the first rows of the CSVs they
# name (the reference_root fixture unpacks them into the reference's layout)
REFERENCE = os.path.join(ROOT, "tests", "golden", "reference")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (HIP kernels on cuda:0)")
    config.addinivalue_line("markers", "slow: long-running test")


def pytest_collection_modifyitems(config, items):
    import torch

    if torch.cuda.is_available():
        return
    skip = pytest.mark.skip(reason="no GPU available")
    for it in items:
        if "gpu" in it.keywords:
            it.add_marker(skip)


@pytest.fixture(scope="session")
def reference_root(tmp_path_factory):
    """A directory laid out like the reference checkout (src/Configuration/*.json,
    Data/<set>/Client-k/<split>/data.csv), unpacked once per session from
    tests/golden/reference (see its README)."""
    import shutil
    import tarfile

    root = tmp_path_factory.mktemp("reference")
    shutil.copytree(os.path.join(REFERENCE, "src"), str(root / "src"))
    for name in sorted(os.listdir(REFERENCE)):
        if name.endswith(".tar.xz"):
            with tarfile.open(os.path.join(REFERENCE, name), "r:xz") as tf:
                tf.extractall(str(root))
    return str(root)
