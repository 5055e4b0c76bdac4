"""Device plumbing: the plain `dev` fixture of the GPU test modules (the ref64 modules take tests/gpu_support.py's, which also prints the
worst observed ratios at teardown).  A test module imports it by name."""
import pytest


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available(), "needs a HIP device"
    yield torch.device("cuda:0")
