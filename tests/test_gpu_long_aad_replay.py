"""tests/cpp_aad/aad_replay.c (built by __graft_entry__.build()): the C calls go/crypto/aes_gpu.go makes
for Encrypt / Decrypt with additional data longer than 4 bytes, checked against the oracle, in ONE child
process."""
import os
import subprocess

import pytest

from conftest import ROOT

BIN = os.path.join(ROOT, "tests", "cpp_aad", "aad_replay")


@pytest.mark.gpu
def test_go_shim_long_additional_replay():
    if not os.path.exists(BIN):
        pytest.fail(f"{BIN} is missing: build it with __graft_entry__.build()")
    r = subprocess.run([BIN, "TestAESAdditional"], capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out
    assert "--- PASS: TestAESAdditional" in out, out
