"""CPU: the nonce generator's host side (quantum_amd/csrc/nonce_rng.h, include/qgcm.h qgcm_nonce_fill /
qgcm_nonce_seed / QGCM_NONCES_GENERATE).  tools/nonce_rng_check.cpp is built with g++ under the address and
undefined-behaviour sanitizers and run: it prints the round keys it expanded (compared here with the
oracle's FIPS-197 expansion) and sweeps the 128-bit counter arithmetic and the reseed rule.  Then the header
defines, the Python bindings and the NULL-context refusals.  No GPU calls."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT
from oracle import oracle as O

KEYS = {
    "zero": bytes(32),
    "fips197_c3": bytes(range(32)),
    "sp800_38a_f55": bytes.fromhex("603deb1015ca71be2b73aef0857d77811f352c073b6108d72d9810a30914dff4"),
}


@pytest.fixture(scope="module")
def tool_output(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("nonce_rng") / "nonce_rng_check"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", os.path.join(ROOT, "tools", "nonce_rng_check.cpp"), "-lpthread", "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)
    r = subprocess.run([str(exe), *[k.hex() for k in KEYS.values()]], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    return r


def test_tool_runs_clean_under_sanitizers(tool_output):
    r = tool_output
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "ERROR: AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    assert "FAIL" not in r.stdout, r.stdout[-4000:]
    m = re.search(r"nonce_rng_check: (\d+) checks, (\d+) failures", r.stdout)
    assert m and int(m.group(1)) > 1000 and int(m.group(2)) == 0, r.stdout[-2000:]


@pytest.mark.parametrize("name", list(KEYS))
def test_round_keys_match_oracle(tool_output, name):
    key = KEYS[name]
    lines = dict(re.findall(r"^rk ([0-9a-f]{64}) ([0-9a-f]{480})$", tool_output.stdout, flags=re.M))
    assert key.hex() in lines, tool_output.stdout[:2000]
    assert bytes.fromhex(lines[key.hex()]) == O.aes256_expand(key)


def test_fips197_c3_last_round_key(tool_output):
    """FIPS-197 A.3 lists the expansion of 603deb10... (w59 = 706c631e); C.3's key 00..1f ends in w56..w59 =
    24fc79cc bf0979e9 371ac23c 6d68de36 (the last round key of the C.3 example)."""
    lines = dict(re.findall(r"^rk ([0-9a-f]{64}) ([0-9a-f]{480})$", tool_output.stdout, flags=re.M))
    assert lines[KEYS["sp800_38a_f55"].hex()].endswith("706c631e")
    assert lines[KEYS["fips197_c3"].hex()].endswith("24fc79ccbf0979e9371ac23c6d68de36")


def test_header_defines():
    hdr = open(os.path.join(ROOT, "include", "qgcm.h")).read()
    assert "#define QGCM_NONCES_GENERATE ((const uint8_t *)(uintptr_t)1)" in hdr
    assert re.search(r"int qgcm_nonce_fill\(qgcm_ctx \*ctx, uint8_t \*d_out, uint32_t n, void \*stream\);", hdr)
    assert re.search(r"int qgcm_nonce_seed\(qgcm_ctx \*ctx, const uint8_t key\[32\], const uint8_t counter\[16\]\);", hdr)
    assert "QGCM_NONCE_RESEED" in hdr


def test_bindings():
    import ctypes as C

    from quantum_amd import _lib

    assert "qgcm_nonce_fill" in _lib.EXPORTS and "qgcm_nonce_seed" in _lib.EXPORTS
    assert _lib.NONCES_GENERATE == 1
    L = _lib.lib()
    assert L.qgcm_nonce_fill.argtypes == [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    assert L.qgcm_nonce_seed.argtypes == [C.c_void_p, C.c_char_p, C.c_char_p]
    src = open(os.path.join(ROOT, "quantum_amd", "batch.py")).read()
    for name in ("def nonce_fill(", "def nonce_seed(", "GENERATE = "):
        assert name in src


def test_null_context_refused():
    from quantum_amd import _lib

    L = _lib.lib()
    assert L.qgcm_nonce_fill(None, None, 4, None) == _lib.QGCM_E_ARG
    assert L.qgcm_nonce_fill(None, 16, 4, None) == _lib.QGCM_E_ARG
    assert L.qgcm_nonce_seed(None, bytes(32), bytes(16)) == _lib.QGCM_E_ARG
    assert L.qgcm_nonce_seed(None, None, None) == _lib.QGCM_E_ARG
    # the marker on a NULL context is an argument error like any other nonce pointer there
    assert L.qgcm_seal_uniform(None, None, 0, 0, 0, 0, _lib.NONCES_GENERATE, 4, None, None) == _lib.QGCM_E_ARG
    assert L.qgcm_seal_batch(None, None, None, 0, _lib.NONCES_GENERATE, 4, None, None) == _lib.QGCM_E_ARG
    assert L.qgcm_seal_host(None, None, 0, 0, 0, 0, _lib.NONCES_GENERATE, 4, None) == _lib.QGCM_E_ARG
    assert L.qgcm_compress_seal_host(None, None, 0, 0, None, 0, _lib.NONCES_GENERATE, 4, 1, None) == _lib.QGCM_E_ARG
