import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden")
if GOLDEN not in sys.path:
    sys.path.append(GOLDEN)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def golden():
    return {name[:-4]: np.load(os.path.join(GOLDEN, name))
            for name in os.listdir(GOLDEN) if name.endswith(".npz")}


@pytest.fixture(scope="session")
def orc():
    import oracle
    oracle.lib()
    return oracle


@pytest.fixture(scope="session")
def fast5_dir(tmp_path_factory):
    """tests/golden/fast5 as a directory of whole files: the fixtures above 1 MB are committed in parts (tests/golden/provenance.py)"""
    import provenance
    d = tmp_path_factory.mktemp("fast5")
    for f in provenance.fixture_files("fast5/*.fast5"):
        (d / os.path.basename(f)).write_bytes(provenance.fixture_bytes(f))
    return str(d)
