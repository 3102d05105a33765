"""CPU: tests/cpp_dtls/dtls_san_driver.cpp -- the DTLS record layer's host code (the rules of dtls_core.h, the key
block, the two UDP calls) built with -fsanitize=address,undefined by the host compiler and run as a child process
(never loaded into Python, never on a GPU)."""
import os
import subprocess

from conftest import ROOT


def test_dtls_driver_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "dtls_san_driver")
    make = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp_dtls"), f"BIN={exe}"],
                          capture_output=True, text=True, timeout=600)
    assert make.returncode == 0, make.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert run.returncode == 0 and "dtls_san_driver ok" in run.stdout, (run.stdout + run.stderr)[-4000:]
