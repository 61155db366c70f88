import os
import subprocess
import sys

import pytest
# Before anything loads libdmpp.so: the library needs libamdhip64.so.7, torch's libraries need its bundled copy under the
# name libamdhip64.so, and the loader matches names, not files.  Loaded first, the library pulls in the system ROCm runtime
# and torch then adds a second HIP runtime to the process; whichever of the two opens the GPU first keeps it, and the other
# reports "no ROCm-capable device" (a suite that asks torch.cuda.is_available() before creating a planner fails).  With
# torch first, libamdhip64.so.7 is already loaded and the library binds to it: one runtime per test process.
import torch  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def oracle():
    """The CPU oracle (test infrastructure). Built on demand with gcc."""
    so = os.path.join(ROOT, "oracle", "liboracle.so")
    srcs = [os.path.join(ROOT, "oracle", f) for f in ("dmpp_oracle.c", "dmpp_grid_oracle.c", "dmpp_oracle_batch.c", "dmpp_oracle.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle")])
    import oracle_binding
    return oracle_binding.Oracle(so)


@pytest.fixture(scope="session")
def dm():
    """The product binding; libdmpp.so must already be built (fails loudly otherwise)."""
    import dmpp_amd
    dmpp_amd.load_library()
    return dmpp_amd


def have_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False
