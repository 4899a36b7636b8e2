import os
import shutil
import socket
import tempfile
import uuid
from pathlib import Path

import pytest


def pytest_configure(config):
    config.addinivalue_line(
        "markers", "gpu: needs an MI355X GPU (run with -m gpu on a GPU box)"
    )


@pytest.fixture
def tmp_path():
    """Short per-test directory. AF_UNIX socket paths are capped at ~107
    bytes and most tests bind ipc://{tmp_path}/<name>.ipc, so pytest's own
    $TMPDIR/pytest-of-<user>/pytest-N/<test-name>0 nesting overflows as
    soon as $TMPDIR is deep."""
    base = "/tmp" if os.access("/tmp", os.W_OK | os.X_OK) else None
    path = tempfile.mkdtemp(prefix="dmx-", dir=base)
    yield Path(path)
    shutil.rmtree(path, ignore_errors=True)


@pytest.fixture
def ipc_addr(tmp_path):
    """Unique ipc:// address per test (reference tests use ipc://{tmp_path})."""
    return f"ipc://{tmp_path}/{uuid.uuid4().hex[:8]}.ipc"


@pytest.fixture
def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


@pytest.fixture(autouse=True)
def _quiet_logs(caplog):
    import logging

    logging.getLogger("detectmateservice_amd").setLevel(logging.WARNING)
    yield
