import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIXTURES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fixtures")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (HIP kernels)")
    config.addinivalue_line("markers", "slow: long-running test")


@pytest.fixture
def ref_resource():
    """Path of one of the reference's small configs / schemas, vendored under tests/fixtures."""
    def _p(name):
        v = os.path.join(FIXTURES, name)
        assert os.path.exists(v), f"tests/fixtures/{name} is missing"
        return v
    return _p


def pytest_collection_modifyitems(config, items):
    """``gpu``-marked tests skip (rather than fail) on a host without a HIP device."""
    if gpu_available():
        return
    skip = pytest.mark.skip(reason="no HIP GPU on this host")
    for it in items:
        if "gpu" in it.keywords:
            it.add_marker(skip)


def gpu_available():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.fixture
def cuda():
    if not gpu_available():
        pytest.skip("no GPU")
    import torch
    return torch.device("cuda")
