import os
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")
    # the oracle runs on the CPU: use this job's core share, not the host's core count (a GPU box reports the whole host)
    try:
        import torch
        n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
        torch.set_num_threads(max(1, min(n, int(os.environ.get("UNET_TEST_THREADS", "16")))))
    except Exception:  # pragma: no cover
        pass


@pytest.fixture(autouse=True)
def _default_tuning():
    """kernel-selection switches a test sets (ops.set_knob / ops.set_tuning) end with it: tests that put a switch back to its default value
    still leave a tuning struct behind, and the next test in the same process would not start from the library defaults"""
    yield
    ops = sys.modules.get("unet_amd.ops")      # (looked up, not imported: importing it loads the HIP library)
    if ops is not None:
        ops.set_tuning()


def pytest_collection_modifyitems(config, items):
    """GPU tests are skipped (not failed) when no GPU is visible and `-m gpu` was not requested."""
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except Exception:  # pragma: no cover
        has_gpu = False
    if has_gpu:
        return
    skip = pytest.mark.skip(reason="no GPU visible")
    for it in items:
        if "gpu" in it.keywords:
            it.add_marker(skip)
