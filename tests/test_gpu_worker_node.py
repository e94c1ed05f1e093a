"""Synchronous deflate() / inflate() of the N-API façade from the main thread and two Workers at once, every result
byte-compared: each N-API environment has its own scratch block (tests/host_node_worker_test.js)."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_sync_calls_from_two_workers_and_the_main_thread(gpu):
    node = shutil.which("node")
    if node is None:
        pytest.skip("node is not installed on this box")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "zlib.es_amd", "host")])
    out = subprocess.run([node, os.path.join(ROOT, "tests", "host_node_worker_test.js")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "worker checks passed" in out.stdout
