"""Peer keys derived on the GPU (quantum_amd/csrc/kdf_kernels.hip kdf_pbkdf2_kernel, kdf_core.h;
qgcm_derive_keys_device / qgcm_derive_set_keys / qgcm_group_derive_set_keys / qgcm_kdf_stats).

Expected keys come from hashlib.pbkdf2_hmac("sha512", ...) and tests/golden/kdf.json.  Counts 1, 63, 64, 65
and 130 cover a partial wave, a full wave, a wave plus one lane and three waves with a ragged tail (the
kernel runs one key per lane in 64-lane blocks); iterations 1, 2 and 3 cover U1 alone, the first xor and
the loop's second pass.  A launch at the full 10000 iterations costs a few tenths of a second whatever its
count, so the file makes seven of them: 65 keys against hashlib and the host, the edge inputs, the
derive-and-install, the re-derive, the derivation under traffic and the two group members."""
import ctypes as C
import hashlib
import random
import threading

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

ITERS = 10000
MAX_KEYS = 80


def pbkdf2(secret: bytes, salt: bytes, iters: int = ITERS) -> bytes:
    return hashlib.pbkdf2_hmac("sha512", secret, salt, iters, 32)


def pairs(n: int, seed: int):
    rng = random.Random(seed)
    return rng.randbytes(32 * n), rng.randbytes(32 * n)


def want_keys(secrets: bytes, salts: bytes, iters: int = ITERS) -> bytes:
    return b"".join(pbkdf2(secrets[i:i + 32], salts[i:i + 32], iters) for i in range(0, len(secrets), 32))


@pytest.fixture(scope="module")
def torch():
    import torch as T

    if not T.cuda.is_available():
        pytest.skip("no GPU")
    return T


@pytest.fixture(scope="module")
def table65():
    """65 secret / salt pairs and their hashlib keys, computed once for the tests that install them."""
    secrets, salts = pairs(65, 0xD0)
    return secrets, salts, want_keys(secrets, salts)


def make_ctx(monkeypatch, device_min, max_keys=MAX_KEYS):
    from quantum_amd.crypto import Context

    if device_min is None:
        monkeypatch.delenv("QGCM_KDF_DEVICE_MIN", raising=False)
    else:
        monkeypatch.setenv("QGCM_KDF_DEVICE_MIN", str(device_min))
    return Context(device=0, max_keys=max_keys)


def seal_check(torch, ctx, slot_keys: dict, unset=(), seed=1):
    """Seals one 33-B and one 1350-B packet under every slot of slot_keys (and one 33-B packet under every
    slot of `unset`) with seal_batch and explicit nonces: the set slots' bytes equal the oracle's under
    the given keys with status 1, the unset slots' packets come back untouched with status 0.  Returns the
    arena bytes."""
    from quantum_amd import batch

    rng = random.Random(seed)
    slots = sorted(slot_keys)
    recs = [(s, L) for s in slots for L in (33, 1350)] + [(s, 33) for s in unset]
    n, nset, stride = len(recs), 2 * len(slots), 1392
    plain = np.frombuffer(rng.randbytes(n * stride), np.uint8).copy()
    nonces = np.frombuffer(rng.randbytes(12 * n), np.uint8).copy()
    offs = np.arange(n, dtype=np.uint64) * np.uint64(stride)
    lens = np.array([L for _, L in recs], np.uint32)
    kidx = np.array([s for s, _ in recs], np.uint32)
    arena = torch.from_numpy(plain.copy()).cuda()
    status = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    batch.seal_batch(ctx, arena, batch.make_descs(offs, lens, kidx, "cuda"), n, torch.from_numpy(nonces).cuda(),
                     status=status)
    got, st = arena.cpu().numpy(), status.cpu().numpy()
    table = bytearray(32 * (int(kidx.max()) + 1))
    for s, k in slot_keys.items():
        table[32 * s:32 * s + 32] = k
    ref = plain.copy()
    O.aesgo_seal_descs(bytes(table), ref, offs[:nset].copy(), lens[:nset].copy(), kidx[:nset].copy(), nonces, 4)
    assert (st[:nset] == 1).all() and (st[nset:] == 0).all(), st.tolist()
    assert np.array_equal(got, ref)
    return got


def round_trip(ctx, slot: int, key: bytes, n: int = 200, seed: int = 5) -> int:
    """n seal_one / open_one round trips on `slot`, each seal checked against the oracle; returns how many
    verified."""
    from quantum_amd import _lib

    L = _lib.lib()
    rng = random.Random(seed)
    good = 0
    for i in range(n):
        ln = (1, 33, 1350)[i % 3]
        pt, nonce, aad = rng.randbytes(ln), rng.randbytes(12), bytes([10, 99, 0, i & 255])
        buf = (C.c_uint8 * (ln + 28)).from_buffer_copy(pt + bytes(28))
        ref = bytearray(pt + bytes(28))
        O.aesgo_encrypt(key, ref, ln, aad, nonce)
        ok = L.qgcm_seal_one(ctx.handle, slot, buf, ln, aad, 4, nonce) == ln + 28 and bytes(buf) == bytes(ref)
        ok = ok and L.qgcm_open_one(ctx.handle, slot, buf, ln + 28, aad, 4) == ln and bytes(buf)[:ln] == pt
        good += bool(ok)
    return good


@pytest.mark.parametrize("count", [1, 63, 64, 65, 130])
def test_low_iteration_counts_vs_hashlib(torch, ctx, count):
    from quantum_amd import crypto

    secrets, salts = pairs(count, 0xA0 + count)
    for iters in (1, 2, 3):
        assert crypto.derive_keys_device(ctx, secrets, salts, iters) == want_keys(secrets, salts, iters), iters


def test_full_iteration_count_vs_hashlib_and_host(torch, ctx, table65):
    from quantum_amd import crypto

    secrets, salts, want = table65
    before = ctx.kdf_stats()
    got = crypto.derive_keys_device(ctx, secrets, salts)
    assert got == want
    assert got == crypto.derive_keys(secrets, salts)  # qgcm_derive_keys, the host pool
    after = ctx.kdf_stats()
    assert after["device_keys"] - before["device_keys"] == 65 and after["launches"] - before["launches"] == 1
    assert after["host_keys"] == before["host_keys"] and after["install_passes"] == before["install_passes"]


def test_edge_inputs(torch, ctx, kdf):
    """All-00 and all-ff secrets and salts (carries across the 32-bit halves, the big-endian output) and
    the committed pbkdf2_path vector in lane 0 and in lane 64 (the second wave)."""
    from quantum_amd import crypto

    p = kdf["pbkdf2_path"]
    ps, pc = p["secret"].encode(), bytes.fromhex(p["salt"])
    z, f = bytes(32), b"\xff" * 32
    rows = [(ps, pc), (z, z), (f, f), (z, f), (f, z)] + [(bytes([i]) * 32, bytes([255 - i]) * 32) for i in range(5, 64)]
    rows.append((ps, pc))  # lane 64
    secrets, salts = b"".join(r[0] for r in rows), b"".join(r[1] for r in rows)
    got = crypto.derive_keys_device(ctx, secrets, salts)
    assert got[:32].hex() == p["out"] and got[64 * 32:65 * 32].hex() == p["out"]
    assert got == want_keys(secrets, salts)
    for iters in (1, 2, 3):
        assert crypto.derive_keys_device(ctx, secrets[:5 * 32], salts[:5 * 32], iters) == \
            want_keys(secrets[:5 * 32], salts[:5 * 32], iters)


def test_iters_bounds_and_argument_order(torch, ctx):
    from quantum_amd import _lib

    L = _lib.lib()
    secrets, salts = pairs(3, 0xB0)
    for bad in (0, (1 << 20) + 1):
        out = C.create_string_buffer(b"\xaa" * 96, 96)
        assert L.qgcm_derive_keys_device(ctx.handle, secrets, salts, 3, bad, out) == _lib.QGCM_E_ARG
        assert out.raw == b"\xaa" * 96
    out = C.create_string_buffer(b"\xaa" * 96, 96)
    assert L.qgcm_derive_keys_device(ctx.handle, None, salts, 3, 1, out) == _lib.QGCM_E_ARG
    assert L.qgcm_derive_keys_device(ctx.handle, secrets, salts, 3, 1, None) == _lib.QGCM_E_ARG
    assert L.qgcm_derive_keys_device(ctx.handle, None, None, 0, 0, None) == _lib.QGCM_OK  # count 0 before iters
    assert out.raw == b"\xaa" * 96
    assert L.qgcm_derive_set_keys(ctx.handle, 0, 1, None, salts) == _lib.QGCM_E_ARG
    assert L.qgcm_derive_set_keys(ctx.handle, ctx.max_keys, 0, None, None) == _lib.QGCM_OK
    assert L.qgcm_derive_set_keys(ctx.handle, ctx.max_keys, 1, None, None) == _lib.QGCM_E_ARG  # NULL before the range
    st = (C.c_uint64 * 8)()
    assert L.qgcm_kdf_stats(ctx.handle, st, 8) == 4 and L.qgcm_kdf_stats(ctx.handle, st, 2) == 2
    assert L.qgcm_kdf_stats(ctx.handle, None, 4) == -1


def test_device_derive_and_install_then_rederive(torch, monkeypatch, table65):
    from quantum_amd import _lib
    from quantum_amd.crypto import Context

    secrets, salts, want = table65
    dev = make_ctx(monkeypatch, 1)
    other = Context(device=0, max_keys=MAX_KEYS)
    try:
        dev.derive_set_keys(3, secrets, salts)
        assert dev.kdf_stats() == {"device_keys": 65, "host_keys": 0, "launches": 1, "install_passes": 1}
        keys = {3 + i: want[32 * i:32 * i + 32] for i in range(65)}
        got = seal_check(torch, dev, keys, unset=(2, 68))
        other.set_keys(3, want)
        assert np.array_equal(got, seal_check(torch, other, keys, unset=(2, 68)))
        assert dev.alloc_slot() == 68  # the slots are reserved as set_keys reserves them
        # the resident per-packet service was ended by the install and starts again
        assert round_trip(dev, 3 + 64, keys[3 + 64], n=6) == 6
        assert dev.resident_stats()["broken"] == 0
        # a range past max_keys: refused before anything is derived or installed
        before = dev.kdf_stats()
        s2, c2 = pairs(4, 0xD1)
        assert _lib.lib().qgcm_derive_set_keys(dev.handle, MAX_KEYS - 3, 4, s2, c2) == _lib.QGCM_E_KEY
        with pytest.raises(_lib.QgcmError):
            dev.derive_set_keys(MAX_KEYS - 3, s2, c2)
        assert dev.kdf_stats() == before
        seal_check(torch, dev, {3: keys[3]}, unset=(MAX_KEYS - 3, MAX_KEYS - 2, MAX_KEYS - 1), seed=2)
        # re-derive over live slots 3..7: packets sealed under the old keys no longer open, new ones do
        L = _lib.lib()
        old = {}
        for s in range(3, 8):
            buf = (C.c_uint8 * (100 + 28))(*range(100))
            assert L.qgcm_seal_one(dev.handle, s, buf, 100, None, 0, None) == 128
            old[s] = bytes(buf)
        s3, c3 = pairs(5, 0xD2)
        dev.derive_set_keys(3, s3, c3)
        new = {3 + i: pbkdf2(s3[32 * i:32 * i + 32], c3[32 * i:32 * i + 32]) for i in range(5)}
        assert all(new[s] != keys[s] for s in new)
        for s in range(3, 8):
            buf = (C.c_uint8 * 128).from_buffer_copy(old[s])
            assert L.qgcm_open_one(dev.handle, s, buf, 128, None, 0) == -1
        seal_check(torch, dev, {**keys, **new}, seed=3)
        assert round_trip(dev, 5, new[5], n=6) == 6
        st = dev.kdf_stats()
        assert st["device_keys"] == 70 and st["host_keys"] == 0 and st["install_passes"] == 2 and st["launches"] == 2
    finally:
        dev.close()
        other.close()


def test_host_path_installs_the_same_bytes(torch, monkeypatch, table65):
    secrets, salts, want = table65
    host = make_ctx(monkeypatch, 0)
    try:
        host.derive_set_keys(3, secrets, salts)
        assert host.kdf_stats() == {"device_keys": 0, "host_keys": 65, "launches": 0, "install_passes": 1}
        seal_check(torch, host, {3 + i: want[32 * i:32 * i + 32] for i in range(65)}, unset=(2, 68))
        assert round_trip(host, 10, want[32 * 7:32 * 8], n=6) == 6
    finally:
        host.close()


def test_below_the_default_threshold_takes_the_host(torch, monkeypatch):
    """The default QGCM_KDF_DEVICE_MIN (gcm_internal.h kKdfDeviceMin): a multiple of 64; one key below it is
    derived on the host.  (The device side of the threshold is the QGCM_KDF_DEVICE_MIN=1 tests' path.)"""
    import os
    import re

    from conftest import ROOT

    src = open(os.path.join(ROOT, "quantum_amd", "csrc", "gcm_internal.h")).read()
    dflt = int(re.search(r"constexpr uint32_t kKdfDeviceMin = (\d+);", src).group(1))
    assert dflt >= 64 and dflt % 64 == 0
    c = make_ctx(monkeypatch, None, max_keys=8)
    try:
        s, salt = pairs(2, 0xD3)
        c.derive_set_keys(1, s, salt)
        assert c.kdf_stats() == {"device_keys": 0, "host_keys": 2, "launches": 0, "install_passes": 1}
        seal_check(torch, c, {1: pbkdf2(s[:32], salt[:32]), 2: pbkdf2(s[32:], salt[32:])}, unset=(0, 3))
    finally:
        c.close()


def test_traffic_during_derivation(torch, monkeypatch):
    """The derivation holds none of the context's I/O locks: 200 per-packet round trips on slot 0 run while
    64 keys are derived for slots 8..71 and installed."""
    dev = make_ctx(monkeypatch, 1)
    try:
        key0 = bytes(range(32))
        dev.set_key(0, key0)
        secrets, salts = pairs(64, 0xD4)
        want = want_keys(secrets, salts)
        result = {}
        t = threading.Thread(target=lambda: result.update(good=round_trip(dev, 0, key0, n=200)))
        t.start()
        dev.derive_set_keys(8, secrets, salts)
        t.join()
        assert result["good"] == 200
        keys = {8 + i: want[32 * i:32 * i + 32] for i in range(64)}
        keys[0] = key0
        seal_check(torch, dev, keys, unset=(7, 72))
        assert dev.kdf_stats()["device_keys"] == 64 and dev.resident_stats()["broken"] == 0
    finally:
        dev.close()


def test_group_derive_set_keys(torch, monkeypatch):
    from quantum_amd import _lib, batch, shard

    monkeypatch.setenv("QGCM_KDF_DEVICE_MIN", "1")
    grp = shard.Group([0, 0], max_keys=64)
    try:
        nkeys = 40
        secrets, salts = pairs(nkeys, 0xD5)
        want = want_keys(secrets, salts)
        grp.derive_set_keys(0, secrets, salts)
        owners = shard.key_shard(np.arange(nkeys), 2)
        members = [grp.member(0), grp.member(1)]
        for m in (0, 1):
            st = members[m].kdf_stats()
            assert st["install_passes"] == 1 and st["device_keys"] == int((owners == m).sum()) and st["host_keys"] == 0
        # a host batch over all 40 keys through the group
        rng = np.random.default_rng(0xD6)
        n = 160
        lens = ((np.arange(n) * 37) % 1400 + 1).astype(np.uint32)
        kidx = (np.arange(n) % nkeys).astype(np.uint32)
        offs = (np.arange(n, dtype=np.uint64) * np.uint64(1440)).astype(np.uint64)
        size = n * 1440
        ptr = _lib.lib().qgcm_host_alloc(size)
        assert ptr
        try:
            harena = np.frombuffer((C.c_uint8 * size).from_address(ptr), np.uint8)
            harena[:] = rng.integers(0, 256, size, dtype=np.uint8)
            nonces = rng.integers(0, 256, 12 * n, dtype=np.uint8)
            ref = harena.copy()
            O.aesgo_seal_descs(want, ref, offs, lens, kidx, nonces, 4)
            status = np.zeros(n, np.uint8)
            assert grp.seal_host(ptr, shard.host_descs(offs, lens, kidx), n, nonces.ctypes.data, 4, status.ctypes.data) == 0
            assert np.array_equal(harena, ref) and (status == 1).all()
            del harena
        finally:
            _lib.lib().qgcm_host_free(ptr)
        # each key lives on its owner only
        for m in (0, 1):
            mine = [k for k in range(nkeys) if owners[k] == m][:3]
            theirs = [k for k in range(nkeys) if owners[k] != m][:3]
            seal_check(torch, members[m], {k: want[32 * k:32 * k + 32] for k in mine}, unset=theirs, seed=7 + m)
    finally:
        grp.close()
