"""CPU: the host side of a peer table keyed from public keys (quantum_amd/csrc/x25519_core.h, include/qgcm.h
qgcm_x25519_batch / qgcm_x25519_device / qgcm_peer_keys_device / qgcm_peers_set_keys /
qgcm_group_peers_set_keys / qgcm_ecdh_stats).  tools/x25519_core_check.cpp is built with g++ under the address
and undefined-behaviour sanitizers and run as a process of its own on a vector file written here from the
host qgcm_x25519 (which tests/test_abi.py pins to RFC 7748 and OpenSSL); then the exports, the bindings, the
argument errors that need no device, and the batched host call against the single one and OpenSSL.  No GPU
calls."""
import ctypes as C
import os
import random
import re
import shutil
import subprocess

import pytest

from conftest import ROOT
from oracle import oracle as O

TOOL = os.path.join(ROOT, "tools", "x25519_core_check.cpp")
# what the tool checks by itself: 10 tobytes(frombytes(x)), 3 x 64 field identities, 8 x 16 + 32 ladders
SELF_CHECKS = 10 + 3 * 64 + 8 * 16 + 32


def vectors(kdf):
    """(scalar, point, expected) rows: the committed RFC 7748 vectors, the alice / bob / shared triple, the
    three peers.first entries, and seeded random pairs through the host qgcm_x25519."""
    from quantum_amd import crypto

    rows = [(bytes.fromhex(v["scalar"]), bytes.fromhex(v["u"]), bytes.fromhex(v["out"])) for v in kdf["x25519"]]
    a, b, nine = kdf["alice"], kdf["bob"], bytes([9]) + bytes(31)
    shared = bytes.fromhex(kdf["shared"])
    rows += [(bytes.fromhex(a["priv"]), nine, bytes.fromhex(a["pub"])),
             (bytes.fromhex(b["priv"]), nine, bytes.fromhex(b["pub"])),
             (bytes.fromhex(a["priv"]), bytes.fromhex(b["pub"]), shared),
             (bytes.fromhex(b["priv"]), bytes.fromhex(a["pub"]), shared)]
    pe = kdf["peers"]
    for f in pe["first"][:3]:
        rows.append((bytes.fromhex(pe["me_priv"]), bytes.fromhex(f["pub"]), bytes.fromhex(f["secret"])))
        rows.append((bytes.fromhex(pe["me_salt"]), bytes.fromhex(f["pubsalt"]), bytes.fromhex(f["salt"])))
    for k, u, want in rows:
        assert crypto.x25519(k, u) == want  # the host path agrees with the committed vectors
    rng = random.Random(0x583235)
    for _ in range(100):
        k, u = rng.randbytes(32), rng.randbytes(32)
        rows.append((k, u, crypto.x25519(k, u)))
    return [f"{k.hex()} {u.hex()} {w.hex()}" for k, u, w in rows]


@pytest.fixture(scope="module")
def tool_output(tmp_path_factory, kdf):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("x25519_core")
    exe, vec = tmp / "x25519_core_check", tmp / "vectors.txt"
    lines = vectors(kdf)
    vec.write_text("# scalar point expected\n" + "\n".join(lines) + "\n")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", TOOL, "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)
    r = subprocess.run([str(exe), str(vec)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    return r, len(lines)


def test_core_check_runs_clean_under_sanitizers(tool_output):
    r, nvec = tool_output
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "ERROR: AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    assert "FAIL" not in r.stdout, r.stdout[-4000:]
    m = re.search(r"x25519_core_check: (\d+) checks, (\d+) failures", r.stdout)
    assert m and int(m.group(2)) == 0 and int(m.group(1)) == nvec + SELF_CHECKS, r.stdout[-2000:]


def test_core_check_catches_a_wrong_vector(tmp_path, kdf):
    """The comparison is live: one flipped bit in an expected output is one failure and a non-zero exit."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / "x25519_core_check"
    subprocess.run(["g++", "-std=c++17", "-O1", TOOL, "-o", str(exe)], check=True, capture_output=True, timeout=300)
    v = kdf["x25519"][0]
    want = bytearray(bytes.fromhex(v["out"]))
    want[31] ^= 1
    vec = tmp_path / "bad.txt"
    vec.write_text(f"{v['scalar']} {v['u']} {v['out']}\n{v['scalar']} {v['u']} {want.hex()}\n")
    r = subprocess.run([str(exe), str(vec)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and re.search(rf"{2 + SELF_CHECKS} checks, 1 failures", r.stdout), r.stdout[-2000:]


NEW = ("qgcm_x25519_batch", "qgcm_x25519_device", "qgcm_peer_keys_device", "qgcm_peers_set_keys",
       "qgcm_group_peers_set_keys", "qgcm_ecdh_stats")


def test_exports_and_bindings():
    from quantum_amd import _lib, crypto, shard

    for name in NEW:
        assert name in _lib.EXPORTS
    L = _lib.lib()
    vp, u8p, u32 = C.c_void_p, C.c_char_p, C.c_uint32
    assert L.qgcm_x25519_batch.argtypes == [u8p, u32, u8p, u32, vp]
    assert L.qgcm_x25519_device.argtypes == [vp, u8p, u32, u8p, u32, vp]
    assert L.qgcm_peer_keys_device.argtypes == [vp, u8p, u8p, u8p, u8p, u32, vp]
    assert L.qgcm_peers_set_keys.argtypes == [vp, u32, u32, u8p, u8p, u8p, u8p]
    assert L.qgcm_group_peers_set_keys.argtypes == [vp, u32, u32, u8p, u8p, u8p, u8p]
    assert L.qgcm_ecdh_stats.argtypes == [vp, vp, C.c_int]
    for f in (crypto.x25519_batch, crypto.x25519_device, crypto.peer_keys_device, crypto.Context.peers_set_keys,
              crypto.Context.ecdh_stats, shard.Group.peers_set_keys):
        assert callable(f)


def test_header_declares_the_calls():
    flat = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "qgcm.h")).read())
    for decl in (
        "int qgcm_x25519_batch(const uint8_t *scalars, uint32_t scalar_stride, const uint8_t *points, uint32_t count, "
        "uint8_t *out);",
        "int qgcm_x25519_device(qgcm_ctx *ctx, const uint8_t *scalars, uint32_t scalar_stride, const uint8_t *points, "
        "uint32_t count, uint8_t *out);",
        "int qgcm_peer_keys_device(qgcm_ctx *ctx, const uint8_t priv_key[32], const uint8_t priv_salt[32], "
        "const uint8_t *pub_keys, const uint8_t *pub_salts, uint32_t count, uint8_t *keys);",
        "int qgcm_peers_set_keys(qgcm_ctx *ctx, uint32_t first_idx, uint32_t count, const uint8_t priv_key[32], "
        "const uint8_t priv_salt[32], const uint8_t *pub_keys, const uint8_t *pub_salts);",
        "int qgcm_group_peers_set_keys(qgcm_group *g, uint32_t first_idx, uint32_t count, const uint8_t priv_key[32], "
        "const uint8_t priv_salt[32], const uint8_t *pub_keys, const uint8_t *pub_salts);",
        "int qgcm_ecdh_stats(const qgcm_ctx *ctx, uint64_t *out, int n);",
    ):
        assert decl in flat, decl


def test_null_arguments_refused():
    from quantum_amd import _lib

    L = _lib.lib()
    s = bytes(32)
    out = C.create_string_buffer(32)
    # NULL context: an argument error whatever else is passed, count 0 included, and before the range check
    assert L.qgcm_peers_set_keys(None, 0, 1, s, s, s, s) == _lib.QGCM_E_ARG
    assert L.qgcm_peers_set_keys(None, 0, 0, s, s, None, None) == _lib.QGCM_E_ARG
    assert L.qgcm_peers_set_keys(None, 1 << 30, 1 << 30, s, s, s, s) == _lib.QGCM_E_ARG
    assert L.qgcm_peer_keys_device(None, s, s, s, s, 1, out) == _lib.QGCM_E_ARG
    assert L.qgcm_peer_keys_device(None, s, s, None, None, 0, None) == _lib.QGCM_E_ARG
    assert L.qgcm_x25519_device(None, s, 0, s, 1, out) == _lib.QGCM_E_ARG
    assert L.qgcm_x25519_device(None, None, 0, None, 0, None) == _lib.QGCM_E_ARG
    assert L.qgcm_group_peers_set_keys(None, 0, 1, s, s, s, s) == _lib.QGCM_E_ARG
    assert L.qgcm_group_peers_set_keys(None, 0, 0, s, s, None, None) == _lib.QGCM_E_ARG
    assert out.raw == bytes(32)
    st = (C.c_uint64 * 3)()
    assert L.qgcm_ecdh_stats(None, st, 3) == -1
    # the host batch: NULL arrays with a count, and strides other than 0 and 32
    assert L.qgcm_x25519_batch(None, 0, s, 1, out) == _lib.QGCM_E_ARG
    assert L.qgcm_x25519_batch(s, 0, None, 1, out) == _lib.QGCM_E_ARG
    assert L.qgcm_x25519_batch(s, 0, s, 1, None) == _lib.QGCM_E_ARG
    for stride in (1, 4, 16, 31, 33, 64):
        assert L.qgcm_x25519_batch(s * 3, stride, s * 2, 2, out) == _lib.QGCM_E_ARG
    assert out.raw == bytes(32)
    assert L.qgcm_x25519_batch(None, 0, None, 0, None) == _lib.QGCM_OK


def test_python_wrappers_check_lengths():
    from quantum_amd import crypto

    with pytest.raises(ValueError):
        crypto.x25519_batch(bytes(32), bytes(33))
    with pytest.raises(ValueError):
        crypto.x25519_batch(bytes(64), bytes(96))  # neither one scalar nor one per point
    with pytest.raises(ValueError):
        crypto.x25519_device(None, bytes(31), bytes(32))
    with pytest.raises(ValueError):
        crypto.peer_keys_device(None, bytes(31), bytes(32), bytes(32), bytes(32))
    with pytest.raises(ValueError):
        crypto.peer_keys_device(None, bytes(32), bytes(32), bytes(64), bytes(32))


@pytest.mark.parametrize("count", [0, 1, 17, 300])
def test_batch_matches_single_calls_and_openssl(count):
    from quantum_amd import _lib, crypto

    L = _lib.lib()
    rng = random.Random(0xB47C + count)
    points, scalars = rng.randbytes(32 * count), rng.randbytes(32 * max(count, 1))
    # one scalar per point
    out = C.create_string_buffer(b"\xaa" * (32 * count + 1), 32 * count + 1)
    assert L.qgcm_x25519_batch(scalars, 32, points, count, out) == _lib.QGCM_OK
    assert out.raw[32 * count:] == b"\xaa"
    for i in range(count):
        k, u = scalars[32 * i:32 * i + 32], points[32 * i:32 * i + 32]
        assert out.raw[32 * i:32 * i + 32] == crypto.x25519(k, u) == O.ossl_x25519(k, u), i
    # one scalar for all
    out = C.create_string_buffer(b"\xaa" * (32 * count + 1), 32 * count + 1)
    assert L.qgcm_x25519_batch(scalars[:32], 0, points, count, out) == _lib.QGCM_OK
    assert out.raw[32 * count:] == b"\xaa"
    for i in range(count):
        u = points[32 * i:32 * i + 32]
        assert out.raw[32 * i:32 * i + 32] == crypto.x25519(scalars[:32], u) == O.ossl_x25519(scalars[:32], u), i
    if count:
        assert crypto.x25519_batch(scalars, points) == b"".join(
            crypto.x25519(scalars[32 * i:32 * i + 32], points[32 * i:32 * i + 32]) for i in range(count))
        assert crypto.x25519_batch(scalars[:32], points) == out.raw[:32 * count]


def test_device_calls_need_a_context():
    """The device calls have no host fallback: without a device there is no context to hand them, and a NULL
    context is an argument error."""
    import torch

    from quantum_amd import _lib

    out = C.create_string_buffer(32)
    assert _lib.lib().qgcm_x25519_device(None, bytes(32), 0, bytes(32), 1, out) == _lib.QGCM_E_ARG
    if torch.cuda.is_available():
        return  # with a device the calls are served: tests/test_gpu_x25519.py
    from quantum_amd.crypto import Context

    with pytest.raises(_lib.QgcmError):
        Context(device=0)
