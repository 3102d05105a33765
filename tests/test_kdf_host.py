"""CPU: the host side of peer keys derived on the GPU (quantum_amd/csrc/kdf_core.h, include/qgcm.h
qgcm_derive_keys_device / qgcm_derive_set_keys / qgcm_group_derive_set_keys / qgcm_kdf_stats).
tools/kdf_core_check.cpp is built with g++ under the address and undefined-behaviour sanitizers and run as a
process of its own on a vector file written here from hashlib; then the exports, the bindings and the
argument errors that need no device.  No GPU calls."""
import ctypes as C
import hashlib
import os
import random
import re
import shutil
import subprocess

import pytest

from conftest import ROOT


def vectors(kdf):
    rng = random.Random(0x4B4446)
    rows = []
    for iters in (1, 2, 3, 5):
        rows += [(rng.randbytes(32), rng.randbytes(32), iters) for _ in range(64)]
    rows += [(rng.randbytes(32), rng.randbytes(32), 10000) for _ in range(6)]
    p = kdf["pbkdf2_path"]
    rows.append((p["secret"].encode(), bytes.fromhex(p["salt"]), p["iters"]))
    lines = [f"{s.hex()} {c.hex()} {it} {hashlib.pbkdf2_hmac('sha512', s, c, it, 32).hex()}" for s, c, it in rows]
    assert lines[-1].endswith(p["out"])  # hashlib agrees with the committed vector
    return lines


@pytest.fixture(scope="module")
def tool_output(tmp_path_factory, kdf):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("kdf_core")
    exe, vec = tmp / "kdf_core_check", tmp / "vectors.txt"
    lines = vectors(kdf)
    vec.write_text("# secret salt iters expected\n" + "\n".join(lines) + "\n")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", os.path.join(ROOT, "tools", "kdf_core_check.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)
    r = subprocess.run([str(exe), str(vec)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    return r, len(lines)


def test_core_check_runs_clean_under_sanitizers(tool_output):
    r, nvec = tool_output
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "ERROR: AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    assert "FAIL" not in r.stdout, r.stdout[-4000:]
    m = re.search(r"kdf_core_check: (\d+) checks, (\d+) failures", r.stdout)
    # every vector line, the sweep (3 iteration counts x (4 + 512) inputs, 3 at 10000) and 2 self-checks
    assert m and int(m.group(2)) == 0 and int(m.group(1)) == nvec + 3 * 516 + 3 + 2, r.stdout[-2000:]


def test_core_check_catches_a_wrong_vector(tool_output, tmp_path):
    """The comparison is live: one flipped bit in an expected key is one failure and a non-zero exit."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / "kdf_core_check"
    subprocess.run(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tools", "kdf_core_check.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=300)
    s, c = bytes(range(32)), bytes(range(32, 64))
    want = bytearray(hashlib.pbkdf2_hmac("sha512", s, c, 2, 32))
    want[31] ^= 1
    vec = tmp_path / "bad.txt"
    vec.write_text(f"{s.hex()} {c.hex()} 2 {want.hex()}\n")
    r = subprocess.run([str(exe), str(vec)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and re.search(r"checks, 1 failures", r.stdout), r.stdout[-2000:]


NEW = ("qgcm_derive_keys_device", "qgcm_derive_set_keys", "qgcm_group_derive_set_keys", "qgcm_kdf_stats")


def test_exports_and_bindings():
    from quantum_amd import _lib, crypto, shard

    for name in NEW:
        assert name in _lib.EXPORTS
    L = _lib.lib()
    vp, u8p, u32 = C.c_void_p, C.c_char_p, C.c_uint32
    assert L.qgcm_derive_keys_device.argtypes == [vp, u8p, u8p, u32, u32, vp]
    assert L.qgcm_derive_set_keys.argtypes == [vp, u32, u32, u8p, u8p]
    assert L.qgcm_group_derive_set_keys.argtypes == [vp, u32, u32, u8p, u8p]
    assert L.qgcm_kdf_stats.argtypes == [vp, vp, C.c_int]
    assert callable(crypto.derive_keys_device) and callable(crypto.Context.derive_set_keys)
    assert callable(crypto.Context.kdf_stats) and callable(shard.Group.derive_set_keys)


def test_header_declares_the_calls():
    hdr = open(os.path.join(ROOT, "include", "qgcm.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    assert ("int qgcm_derive_keys_device(qgcm_ctx *ctx, const uint8_t *secrets, const uint8_t *salts, uint32_t count, "
            "uint32_t iters, uint8_t *keys);") in flat
    assert ("int qgcm_derive_set_keys(qgcm_ctx *ctx, uint32_t first_idx, uint32_t count, const uint8_t *secrets, "
            "const uint8_t *salts);") in flat
    assert ("int qgcm_group_derive_set_keys(qgcm_group *g, uint32_t first_idx, uint32_t count, const uint8_t *secrets, "
            "const uint8_t *salts);") in flat
    assert "int qgcm_kdf_stats(const qgcm_ctx *ctx, uint64_t *out, int n);" in flat
    assert "QGCM_KDF_DEVICE_MIN" in hdr


def test_null_arguments_refused():
    from quantum_amd import _lib

    L = _lib.lib()
    s = bytes(32)
    out = C.create_string_buffer(32)
    # NULL context: an argument error whatever else is passed, count 0 included
    assert L.qgcm_derive_set_keys(None, 0, 1, s, s) == _lib.QGCM_E_ARG
    assert L.qgcm_derive_set_keys(None, 0, 0, None, None) == _lib.QGCM_E_ARG
    assert L.qgcm_derive_set_keys(None, 1 << 30, 1 << 30, s, s) == _lib.QGCM_E_ARG  # before the range check
    assert L.qgcm_derive_keys_device(None, s, s, 1, 10000, out) == _lib.QGCM_E_ARG
    assert L.qgcm_derive_keys_device(None, s, s, 1, 0, out) == _lib.QGCM_E_ARG
    assert L.qgcm_derive_keys_device(None, None, None, 0, 10000, None) == _lib.QGCM_E_ARG
    assert out.raw == bytes(32)
    assert L.qgcm_group_derive_set_keys(None, 0, 1, s, s) == _lib.QGCM_E_ARG
    assert L.qgcm_group_derive_set_keys(None, 0, 0, None, None) == _lib.QGCM_E_ARG
    st = (C.c_uint64 * 4)()
    assert L.qgcm_kdf_stats(None, st, 4) == -1


def test_python_wrappers_check_lengths():
    from quantum_amd import crypto

    with pytest.raises(ValueError):
        crypto.derive_keys_device(None, bytes(33), bytes(33))
    with pytest.raises(ValueError):
        crypto.derive_keys_device(None, bytes(64), bytes(32))


def test_device_derivation_needs_a_context():
    """qgcm_derive_keys_device has no host fallback: without a device there is no context to hand it (the
    context-creation path refuses), and a NULL context is an argument error."""
    import torch

    from quantum_amd import _lib

    out = C.create_string_buffer(32)
    assert _lib.lib().qgcm_derive_keys_device(None, bytes(32), bytes(32), 1, 10000, out) == _lib.QGCM_E_ARG
    if torch.cuda.is_available():
        return  # with a device the call is served: tests/test_gpu_kdf.py
    from quantum_amd.crypto import Context

    with pytest.raises(_lib.QgcmError):
        Context(device=0)
    err = C.create_string_buffer(_lib.ERRLEN)
    assert not _lib.lib().qgcm_create(0, 16, err, _lib.ERRLEN) and err.value
