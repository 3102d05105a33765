"""A peer table keyed from public keys on the GPU (quantum_amd/csrc/x25519_kernels.hip x25519_ladder_kernel,
x25519_core.h; qgcm_x25519_device / qgcm_peer_keys_device / qgcm_peers_set_keys / qgcm_group_peers_set_keys /
qgcm_ecdh_stats).

The yardstick is never the kernel: expected ladders come from OpenSSL (O.ossl_x25519) or, where OpenSSL
refuses the input (an all-zero shared secret), from the host qgcm_x25519, which tests/test_abi.py pins to RFC
7748 and OpenSSL; expected keys come from hashlib.pbkdf2_hmac and tests/golden/kdf.json.  Counts 1, 63, 64,
65 and 130 cover a partial wave, a full wave, a wave plus one lane and three waves with a ragged tail (the
kernel runs one ladder per lane in 64-lane blocks).  A derivation launch at the full 10000 iterations costs
a few tenths of a second whatever its count, so the file makes six of them."""
import ctypes as C
import hashlib
import random
import threading

import numpy as np
import pytest

from oracle import oracle as O
from test_gpu_kdf import MAX_KEYS, make_ctx, pbkdf2, round_trip, seal_check

pytestmark = pytest.mark.gpu

P = 2 ** 255 - 19


def le(x: int) -> bytes:
    return (x % 2 ** 256).to_bytes(32, "little")


@pytest.fixture(scope="module")
def torch():
    import torch as T

    if not T.cuda.is_available():
        pytest.skip("no GPU")
    return T


def host_ladders(scalars: bytes, points: bytes) -> bytes:
    """Per-lane host qgcm_x25519 (scalars: 32 bytes for all lanes or 32 per lane)."""
    from quantum_amd import crypto

    n = len(points) // 32
    return b"".join(crypto.x25519(scalars[32 * i:32 * i + 32] if len(scalars) > 32 else scalars,
                                  points[32 * i:32 * i + 32]) for i in range(n))


def ossl_ladders(scalars: bytes, points: bytes) -> bytes:
    n = len(points) // 32
    return b"".join(O.ossl_x25519(scalars[32 * i:32 * i + 32] if len(scalars) > 32 else scalars,
                                  points[32 * i:32 * i + 32]) for i in range(n))


@pytest.fixture(scope="module")
def table65():
    """This node's private key and salt, 65 peers' public keys and salts, and the keys of
    common/mapping.go:90-99 by OpenSSL's ladders and hashlib, computed once for the tests that use them."""
    rng = random.Random(0xE0)
    priv_key, priv_salt = rng.randbytes(32), rng.randbytes(32)
    pub_keys = b"".join(O.ossl_x25519_base(rng.randbytes(32)) for _ in range(65))
    pub_salts = b"".join(O.ossl_x25519_base(rng.randbytes(32)) for _ in range(65))
    secrets, salts = ossl_ladders(priv_key, pub_keys), ossl_ladders(priv_salt, pub_salts)
    keys = b"".join(pbkdf2(secrets[i:i + 32], salts[i:i + 32]) for i in range(0, 65 * 32, 32))
    return priv_key, priv_salt, pub_keys, pub_salts, keys


@pytest.mark.parametrize("count", [1, 63, 64, 65, 130])
def test_ladder_bytes_vs_openssl(torch, ctx, count):
    from quantum_amd import crypto

    rng = random.Random(0xC0 + count)
    scalars, points = rng.randbytes(32 * count), rng.randbytes(32 * count)
    before = ctx.ecdh_stats()
    assert crypto.x25519_device(ctx, scalars, points) == ossl_ladders(scalars, points)  # a scalar per lane
    assert crypto.x25519_device(ctx, scalars[:32], points) == ossl_ladders(scalars[:32], points)  # one for all
    after = ctx.ecdh_stats()
    assert after["device"] - before["device"] == 2 * count and after["launches"] - before["launches"] == 2
    assert after["host"] == before["host"]


def test_edge_inputs_with_mixed_neighbours(torch, ctx, kdf):
    """Edge points and edge scalars, every pair, each between two random pairs so that no wave holds edge
    inputs alone; per-lane scalars.  Compared with the host qgcm_x25519; an all-zero shared secret is
    returned, not refused."""
    from quantum_amd import crypto

    order8 = [325606250916557431795983626356110631294008115727848805560023387167927233504,
              39382357235489614581723060781553021112529911719440698176882885853963445705823]
    points = [le(x) for x in (0, 1, 9, P - 1, P, P + 1, 2 ** 255 - 1, 2 ** 256 - 1, *order8, 2 * P - 1, 2 * P, 2 * P + 1)]
    scalars = [bytes(32), b"\xff" * 32, le(1), le(1 << 254), le(1 << 255)]
    rng = random.Random(0xC9)
    rows = []
    for k in scalars:
        for u in points:
            rows += [(rng.randbytes(32), rng.randbytes(32)), (k, u)]
    for v in kdf["x25519"]:
        rows.append((bytes.fromhex(v["scalar"]), bytes.fromhex(v["u"])))
    a, b = kdf["alice"], kdf["bob"]
    rows += [(bytes.fromhex(a["priv"]), bytes.fromhex(b["pub"])), (bytes.fromhex(b["priv"]), bytes.fromhex(a["pub"]))]
    ks, us = b"".join(r[0] for r in rows), b"".join(r[1] for r in rows)
    assert len(rows) > 128  # more than two waves
    got = crypto.x25519_device(ctx, ks, us)
    want = host_ladders(ks, us)
    for i in range(len(rows)):
        assert got[32 * i:32 * i + 32] == want[32 * i:32 * i + 32], (i, rows[i][0].hex(), rows[i][1].hex())
    n = len(rows)
    nv = len(kdf["x25519"])
    for j, v in enumerate(kdf["x25519"]):
        i = n - 2 - nv + j
        assert got[32 * i:32 * i + 32].hex() == v["out"]
    assert got[32 * (n - 2):32 * (n - 1)].hex() == kdf["shared"] and got[32 * (n - 1):].hex() == kdf["shared"]
    # the small-order points give the all-zero secret under every scalar: rows 1, 3, 5, ... are the edge pairs
    zero_points = set(points[:2] + points[3:6] + points[8:10])
    zeros = [i for i in range(1, 2 * len(scalars) * len(points), 2) if rows[i][1] in zero_points]
    assert len(zeros) == len(scalars) * len(zero_points)
    assert all(got[32 * i:32 * i + 32] == bytes(32) for i in zeros)
    # one shared scalar over the edge points, random neighbours between them
    mixed = b"".join(u + rng.randbytes(32) for u in points)
    for k in scalars:
        assert crypto.x25519_device(ctx, k, mixed) == host_ladders(k, mixed)


def test_iterated_vector(torch, ctx):
    """RFC 7748 s5.2's k <- X25519(k, u), u <- old k for 1000 rounds, as 64 lanes of different starts: lane 0
    starts from k = u = 9 (the RFC's values after 1 and 1000 rounds), the others from random pairs.  Each
    round is one device call of count 64; the host runs the same chain with qgcm_x25519_batch."""
    from quantum_amd import crypto

    rng = random.Random(0xCA)
    k = le(9) + rng.randbytes(32 * 63)
    u = le(9) + rng.randbytes(32 * 63)
    hk, hu = k, u
    for rnd in range(1, 1001):
        k, u = crypto.x25519_device(ctx, k, u), k
        if rnd == 1:
            assert k == host_ladders(hk, hu)
            assert k[:32].hex() == "422c8e7a6227d7bca1350b3e2bb7279f7897b87bb6854b783c60e80311ae3079"
    for rnd in range(1000):
        hk, hu = crypto.x25519_batch(hk, hu), hk
    assert k == hk and u == hu
    assert k[:32].hex() == "684cf59ba83309552800ef566f2f4d3c1c3887c49360e3875f2eb94d99532c51"


def test_pipeline_bytes_65_peers(torch, ctx, table65):
    from quantum_amd import crypto

    priv_key, priv_salt, pub_keys, pub_salts, want = table65
    kb, eb = ctx.kdf_stats(), ctx.ecdh_stats()
    assert crypto.peer_keys_device(ctx, priv_key, priv_salt, pub_keys, pub_salts) == want
    ka, ea = ctx.kdf_stats(), ctx.ecdh_stats()
    # one ladder launch over both halves, one derivation launch
    assert ea["device"] - eb["device"] == 130 and ea["launches"] - eb["launches"] == 1 and ea["host"] == eb["host"]
    assert ka["device_keys"] - kb["device_keys"] == 65 and ka["launches"] - kb["launches"] == 1
    assert ka["host_keys"] == kb["host_keys"] and ka["install_passes"] == kb["install_passes"]


def test_pipeline_peer_table_digest(torch, ctx, kdf):
    """The 1024-peer recipe of kdf.json: public values are x25519_base of the seeded privates."""
    from quantum_amd import crypto

    pe = kdf["peers"]
    me_priv, me_salt = bytes.fromhex(pe["me_priv"]), bytes.fromhex(pe["me_salt"])
    privs = b"".join(O.stream_bytes(pe["seed_peers"], 64 * i, 32) for i in range(1024))
    salts = b"".join(O.stream_bytes(pe["seed_peers"], 64 * i + 32, 32) for i in range(1024))
    nine = le(9)
    pub_keys, pub_salts = crypto.x25519_batch(privs, nine * 1024), crypto.x25519_batch(salts, nine * 1024)
    for f in pe["first"]:
        i = f["index"]
        assert pub_keys[32 * i:32 * i + 32].hex() == f["pub"] and pub_salts[32 * i:32 * i + 32].hex() == f["pubsalt"]
    eb, kb = ctx.ecdh_stats(), ctx.kdf_stats()
    keys = crypto.peer_keys_device(ctx, me_priv, me_salt, pub_keys, pub_salts)
    for f in pe["first"]:
        i = f["index"]
        assert keys[32 * i:32 * i + 32].hex() == f["key"]
    assert hashlib.sha256(keys).hexdigest() == pe["sha256_of_1024_keys"]
    ea, ka = ctx.ecdh_stats(), ctx.kdf_stats()
    assert ea["device"] - eb["device"] == 2048 and ea["launches"] - eb["launches"] == 1
    assert ka["device_keys"] - kb["device_keys"] == 1024 and ka["launches"] - kb["launches"] == 1


def test_install_device_and_host_paths(torch, monkeypatch, table65):
    priv_key, priv_salt, pub_keys, pub_salts, want = table65
    keys = {3 + i: want[32 * i:32 * i + 32] for i in range(65)}
    probe = {s: keys[s] for s in (3, 3 + 63, 3 + 64)}  # lanes 0, 63 and 64 (the last)
    dev = make_ctx(monkeypatch, 1)
    try:
        dev.peers_set_keys(3, priv_key, priv_salt, pub_keys, pub_salts)
        assert dev.ecdh_stats() == {"device": 130, "host": 0, "launches": 1}
        assert dev.kdf_stats() == {"device_keys": 65, "host_keys": 0, "launches": 1, "install_passes": 1}
        got_all = seal_check(torch, dev, keys, unset=(2, 68))
        got = seal_check(torch, dev, probe, unset=(2, 68), seed=2)
        assert dev.alloc_slot() == 68  # the slots are reserved as set_keys reserves them
        assert round_trip(dev, 3 + 64, keys[3 + 64], n=6) == 6 and dev.resident_stats()["broken"] == 0
    finally:
        dev.close()
    host = make_ctx(monkeypatch, 0)
    try:
        host.peers_set_keys(3, priv_key, priv_salt, pub_keys, pub_salts)
        assert host.ecdh_stats() == {"device": 0, "host": 130, "launches": 0}
        assert host.kdf_stats() == {"device_keys": 0, "host_keys": 65, "launches": 0, "install_passes": 1}
        assert np.array_equal(got_all, seal_check(torch, host, keys, unset=(2, 68)))
        assert np.array_equal(got, seal_check(torch, host, probe, unset=(2, 68), seed=2))
    finally:
        host.close()


def test_refusals_draw_nothing(torch, monkeypatch):
    from quantum_amd import _lib

    L = _lib.lib()
    rng = random.Random(0xE1)
    dev = make_ctx(monkeypatch, 1)
    try:
        key0 = rng.randbytes(32)
        dev.set_key(0, key0)
        first = seal_check(torch, dev, {0: key0}, unset=(1,))
        s, pubs = rng.randbytes(32), rng.randbytes(32 * 4)
        kb, eb = dev.kdf_stats(), dev.ecdh_stats()
        assert L.qgcm_peers_set_keys(dev.handle, MAX_KEYS - 3, 4, s, s, pubs, pubs) == _lib.QGCM_E_KEY
        assert L.qgcm_peers_set_keys(dev.handle, 0, MAX_KEYS + 1, s, s, pubs, pubs) == _lib.QGCM_E_KEY
        with pytest.raises(_lib.QgcmError):
            dev.peers_set_keys(MAX_KEYS - 3, s, s, pubs, pubs)
        # NULL before the range, the range before count 0's OK
        assert L.qgcm_peers_set_keys(dev.handle, MAX_KEYS, 1, s, s, None, pubs) == _lib.QGCM_E_ARG
        assert L.qgcm_peers_set_keys(dev.handle, 0, 1, None, s, pubs, pubs) == _lib.QGCM_E_ARG
        assert L.qgcm_peers_set_keys(dev.handle, MAX_KEYS + 1, 0, s, s, None, None) == _lib.QGCM_E_KEY
        assert L.qgcm_peers_set_keys(dev.handle, MAX_KEYS, 0, s, s, None, None) == _lib.QGCM_OK
        out = C.create_string_buffer(b"\xaa" * 128, 128)
        assert L.qgcm_x25519_device(dev.handle, s, 16, pubs, 4, out) == _lib.QGCM_E_ARG  # stride 0 or 32 only
        assert L.qgcm_x25519_device(dev.handle, None, 0, pubs, 4, out) == _lib.QGCM_E_ARG
        assert L.qgcm_x25519_device(dev.handle, None, 0, None, 0, None) == _lib.QGCM_OK
        assert L.qgcm_peer_keys_device(dev.handle, s, s, None, pubs, 4, out) == _lib.QGCM_E_ARG
        assert L.qgcm_peer_keys_device(dev.handle, s, s, None, None, 0, None) == _lib.QGCM_OK
        assert out.raw == b"\xaa" * 128
        assert dev.kdf_stats() == kb and dev.ecdh_stats() == eb
        st = (C.c_uint64 * 8)()
        assert L.qgcm_ecdh_stats(dev.handle, st, 8) == 3 and L.qgcm_ecdh_stats(dev.handle, st, 2) == 2
        assert L.qgcm_ecdh_stats(dev.handle, None, 3) == -1
        # the slot installed before still seals as before, the refused ranges hold no key
        assert np.array_equal(first, seal_check(torch, dev, {0: key0}, unset=(1,)))
        seal_check(torch, dev, {0: key0}, unset=(MAX_KEYS - 3, MAX_KEYS - 2, MAX_KEYS - 1), seed=2)
    finally:
        dev.close()


def test_traffic_during_peers_set_keys(torch, monkeypatch, table65):
    """The ladders and the derivation hold none of the context's I/O locks: 200 per-packet round trips on slot
    0 run while 64 peers' keys are computed for slots 8..71 and installed."""
    priv_key, priv_salt, pub_keys, pub_salts, want = table65
    dev = make_ctx(monkeypatch, 1)
    try:
        key0 = bytes(range(32))
        dev.set_key(0, key0)
        result = {}
        t = threading.Thread(target=lambda: result.update(good=round_trip(dev, 0, key0, n=200)))
        t.start()
        try:
            dev.peers_set_keys(8, priv_key, priv_salt, pub_keys[:64 * 32], pub_salts[:64 * 32])
        finally:
            t.join()  # on every path: the context must not be closed under the thread's calls
        assert result["good"] == 200
        keys = {8 + i: want[32 * i:32 * i + 32] for i in range(64)}
        keys[0] = key0
        seal_check(torch, dev, keys, unset=(7, 72))
        assert dev.ecdh_stats() == {"device": 128, "host": 0, "launches": 1}
        assert dev.kdf_stats()["device_keys"] == 64 and dev.resident_stats()["broken"] == 0
    finally:
        dev.close()


def test_group_peers_set_keys(torch, monkeypatch):
    from quantum_amd import shard

    monkeypatch.setenv("QGCM_KDF_DEVICE_MIN", "1")
    rng = random.Random(0xE2)
    npeers = 130
    priv_key, priv_salt = rng.randbytes(32), rng.randbytes(32)
    pub_keys = b"".join(O.ossl_x25519_base(rng.randbytes(32)) for _ in range(npeers))
    pub_salts = b"".join(O.ossl_x25519_base(rng.randbytes(32)) for _ in range(npeers))
    grp = shard.Group([0, 0], max_keys=160)
    try:
        grp.peers_set_keys(5, priv_key, priv_salt, pub_keys, pub_salts)
        owners = shard.key_shard(np.arange(5, 5 + npeers), 2)
        members = [grp.member(0), grp.member(1)]
        for m in (0, 1):
            share = int((owners == m).sum())
            assert share > 0
            assert members[m].ecdh_stats() == {"device": 2 * share, "host": 0, "launches": 1}
            st = members[m].kdf_stats()
            assert st["install_passes"] == 1 and st["device_keys"] == share and st["host_keys"] == 0
        # seals under keys of both members: the first three and the last of each, keys derived independently
        for m in (0, 1):
            mine = [i for i in range(npeers) if owners[i] == m]
            theirs = [5 + i for i in range(npeers) if owners[i] != m][:3]
            keys = {}
            for i in mine[:3] + mine[-1:]:
                secret = O.ossl_x25519(priv_key, pub_keys[32 * i:32 * i + 32])
                salt = O.ossl_x25519(priv_salt, pub_salts[32 * i:32 * i + 32])
                keys[5 + i] = pbkdf2(secret, salt)
            seal_check(torch, members[m], keys, unset=theirs, seed=7 + m)
    finally:
        grp.close()
