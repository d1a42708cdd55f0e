import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs an MI355X (HIP) device")
    config.addinivalue_line("markers", "slow: long-running test")
    config.addinivalue_line("markers", "reference: compares against recorded outputs of the reference (tests/golden)")

@pytest.fixture(scope="session")
def cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from raft_ros_amd.ops import _ext

    assert _ext.is_loaded(), f"native extension must load on the GPU box: {_ext.load_error()}"
    return torch.device("cuda", 0)
