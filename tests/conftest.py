import os
import pathlib
import shutil
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with `-m gpu` on the GPU box)")


@pytest.fixture(scope="session")
def oracle():
    from oracle import pnn_oracle
    pnn_oracle.build()
    return pnn_oracle


# A Unix-domain socket's address holds at most 107 bytes (sockaddr_un.sun_path); pytest's tmp_path under a deep $TMPDIR
# can be longer than that on its own, and the service refuses such a path (PNN_E_ARG).
SOCK_DIR_MAX = 64


@pytest.fixture
def sock_dir(tmp_path):
    """A directory short enough to hold the tests' sockets: tmp_path where it is, else a fresh directory under /tmp."""
    if len(str(tmp_path)) <= SOCK_DIR_MAX:
        yield tmp_path
        return
    d = tempfile.mkdtemp(prefix="pnn-", dir="/tmp")
    try:
        yield pathlib.Path(d)
    finally:
        shutil.rmtree(d, ignore_errors=True)
