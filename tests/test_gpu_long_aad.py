"""Additional data of any length on the per-packet calls (qgcm_seal_one / qgcm_open_one behind
AES.Encrypt / AES.Decrypt; crypto/aes.go:41-62 passes `additional` straight to cipher.AEAD).  Beyond
the record's 4 bytes the additional data travels as a tail of 16-B rows behind the record and the
latency engine hashes ceil(aad_len / 16) blocks of it: checked bit-exact against the oracle on the
resident path and the launch path, in both GHASH forms (flat tables up to 128 exponents, Horner + Estrin
beyond) and at the exponent counts where their bookkeeping changes, with tampering, slot reuse, threads,
and the refusals of include/qgcm.h's size rule."""
import json
import os
import random
import threading

import pytest

from conftest import ROOT
from oracle import oracle as O

pytestmark = pytest.mark.gpu

AAD4 = bytes([10, 99, 0, 1])
THIN_AADS = (5, 17, 64, 1000)
THIN_LENS = (0, 100, 1350)


@pytest.fixture(scope="module")
def torch():
    import torch as T

    if not T.cuda.is_available():
        pytest.skip("no GPU")
    return T


def make_ctx(**env):
    from quantum_amd.crypto import Context

    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return Context(device=0, max_keys=64)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def ctx(torch):
    c = make_ctx()
    yield c
    c.close()


def pair(aes, key, L, aad, rng):
    """Seal against the oracle, open back; None or what went wrong."""
    pt, nonce = rng.randbytes(L), rng.randbytes(12)
    data, want = bytearray(pt + bytes(28)), bytearray(pt + bytes(28))
    n, err = aes.Encrypt(data, L, aad or None, nonce=nonce)
    assert O.aesgo_encrypt(key, want, L, aad, nonce) == L + 28
    if err is not None or n != L + 28:
        return f"seal L={L} aad={len(aad)}: {err}"
    if data != want:
        return f"seal L={L} aad={len(aad)}: bytes differ from the oracle"
    n, err = aes.Decrypt(data, aad or None)
    if err is not None or n != L or bytes(data[:L]) != pt:
        return f"open L={L} aad={len(aad)}: {err}"
    return None


def grid(aes, key, aads, lens, seed):
    rng = random.Random(seed)
    bad = [e for a in aads for L in lens if (e := pair(aes, key, L, rng.randbytes(a), rng))]
    assert not bad, bad[:5]


def test_spec_vector_with_aad(ctx):
    """The SP 800-38D AES-256 vector of tests/golden/gcm_spec.json that carries additional data (20 B,
    60 B of plaintext): ciphertext and tag equal the file's, and it opens."""
    from quantum_amd.crypto import AES

    with open(os.path.join(ROOT, "tests", "golden", "gcm_spec.json")) as f:
        vs = [v for v in json.load(f) if v["aad"]]
    assert vs and all(len(v["aad"]) == 40 and len(v["pt"]) == 120 for v in vs)
    for v in vs:
        aes = AES(bytes.fromhex(v["key"]), ctx=ctx)
        pt, aad = bytes.fromhex(v["pt"]), bytes.fromhex(v["aad"])
        data = bytearray(pt + bytes(28))
        n, err = aes.Encrypt(data, len(pt), aad, nonce=bytes.fromhex(v["iv"]))
        assert err is None and n == len(pt) + 28
        assert data[:len(pt)].hex() == v["ct"] and data[len(pt):len(pt) + 16].hex() == v["tag"]
        n, err = aes.Decrypt(data, aad)
        assert err is None and n == len(pt) and bytes(data[:len(pt)]) == pt


def test_grid_resident(ctx):
    """Every block-edge AAD length against every block-edge payload, each pair served by the resident
    kernel (two requests) and none by a launch."""
    from quantum_amd.crypto import AES

    key = bytes(range(3, 35))
    aes = AES(key, ctx=ctx)
    aads = (0, 1, 4, 5, 13, 15, 16, 17, 31, 32, 33, 64, 1000)
    lens = (0, 1, 15, 16, 17, 100, 1350)
    before = ctx.launch_counts()
    grid(aes, key, aads, lens, 0xA001)
    after = ctx.launch_counts()
    assert after["resident"] - before["resident"] == 2 * len(aads) * len(lens)
    assert after["one"] == before["one"]


@pytest.mark.parametrize("L,aads", [
    (1350, (672, 673)),                  # emax 128, 129: the last flat packet, the first chained one
    (0, (976, 992, 1008, 1009, 1024)),   # emax 62..65: the Estrin top clamp at 63, the first H^64 step
    (2016, (0, 5, 32)),                  # the payload where flat eligibility ended before
])
def test_ghash_form_boundaries(ctx, L, aads):
    from quantum_amd.crypto import AES

    key = bytes(range(11, 43))
    aes = AES(key, ctx=ctx)
    grid(aes, key, aads, (L,), 0xA002 + L)


def test_chained_only_keys(torch):
    """No flat GHASH tables (QGCM_FLAT_GHASH_KEYS=0): every packet takes the Horner + Estrin form."""
    from quantum_amd.crypto import AES

    c = make_ctx(QGCM_FLAT_GHASH_KEYS=0)
    try:
        key = bytes(range(21, 53))
        aes = AES(key, ctx=c)
        before = c.launch_counts()
        grid(aes, key, THIN_AADS, THIN_LENS, 0xA003)
        after = c.launch_counts()
        assert after["resident"] - before["resident"] == 2 * len(THIN_AADS) * len(THIN_LENS)
    finally:
        c.close()


def test_launch_path(torch):
    """QGCM_RESIDENT=0: every call is a gcm_one_kernel launch, the tail in the pinned staging slot."""
    from quantum_amd.crypto import AES

    c = make_ctx(QGCM_RESIDENT=0)
    try:
        key = bytes(range(31, 63))
        aes = AES(key, ctx=c)
        before = c.launch_counts()
        grid(aes, key, THIN_AADS, THIN_LENS, 0xA004)
        after = c.launch_counts()
        assert after["one"] - before["one"] == 2 * len(THIN_AADS) * len(THIN_LENS)
        assert after["resident"] == 0
    finally:
        c.close()


def test_past_the_resident_slot(ctx):
    """9000 B with 8000 B of additional data fit the engine but no 16-KiB resident slot: a launch."""
    from quantum_amd.crypto import AES

    key = bytes(range(41, 73))
    aes = AES(key, ctx=ctx)
    before = ctx.launch_counts()
    rng = random.Random(0xA005)
    assert pair(aes, key, 9000, rng.randbytes(8000), rng) is None
    after = ctx.launch_counts()
    assert after["one"] - before["one"] == 2 and after["resident"] == before["resident"]


def refused(aes, L, aad, rng):
    data = bytearray(rng.randbytes(L + 28))
    before = bytes(data)
    n, err = aes.Encrypt(data, L, aad, nonce=rng.randbytes(12))
    return err is not None and n < 0 and bytes(data) == before


def test_refusals(ctx, torch):
    from quantum_amd.crypto import AES, MaxAdditional

    assert MaxAdditional == 16384
    key = bytes(range(51, 83))
    aes = AES(key, ctx=ctx)
    rng = random.Random(0xA006)
    # over the combined cap, then over QGCM_MAX_AAD at any L; an ordinary call works after each
    for L, a in ((20000, 16384), (0, 16385), (100, 16385), (20000, 16385)):
        assert refused(aes, L, rng.randbytes(a), rng), (L, a)
        assert pair(aes, key, 1350, AAD4, rng) is None
    # just inside the rule: ((4 + L + 28 + 15) & ~15) + 16384 == 32752
    assert pair(aes, key, 16336, rng.randbytes(16384), rng) is None
    assert refused(aes, 16337, rng.randbytes(16384), rng)
    # the A/B knob that forces the batch kernel has no long-AAD form
    c = make_ctx(QGCM_ONE_KERNEL=0)
    try:
        aes0 = AES(key, ctx=c)
        assert refused(aes0, 100, rng.randbytes(5), rng)
        assert pair(aes0, key, 100, AAD4, rng) is None
        data = bytearray(rng.randbytes(128))
        before = bytes(data)
        _, err = aes0.Decrypt(data, rng.randbytes(5))
        assert err is not None and bytes(data) == before
        assert pair(aes0, key, 1350, AAD4, rng) is None
    finally:
        c.close()


def test_tamper(ctx):
    """One flipped bit in the additional data (first byte, last byte, byte 16), the ciphertext, the tag
    or the nonce, and additional data one byte shorter or one zero byte longer (the length block):
    each open fails exactly where the oracle's does, zeroes the plaintext, leaves tag and nonce."""
    from quantum_amd.crypto import AES

    key = bytes(range(61, 93))
    aes = AES(key, ctx=ctx)
    rng = random.Random(0xA007)
    errs = []
    for a in (5, 16, 33, 1000):
        for L in (100, 1350):
            aad, pt, nonce = rng.randbytes(a), rng.randbytes(L), rng.randbytes(12)
            data = bytearray(pt + bytes(28))
            n, err = aes.Encrypt(data, L, aad, nonce=nonce)
            assert err is None and n == L + 28, (a, L, err)
            kinds = ["aad_first", "aad_last", "ct", "tag", "nonce", "aad_short", "aad_long"] + (["aad_16"] if a > 16 else [])
            for kind in kinds:
                bad, bad_aad = bytearray(data), bytearray(aad)
                if kind == "aad_first":
                    bad_aad[0] ^= 1
                elif kind == "aad_last":
                    bad_aad[-1] ^= 0x80
                elif kind == "aad_16":
                    bad_aad[16] ^= 4
                elif kind == "ct":
                    bad[rng.randrange(L)] ^= 0x10
                elif kind == "tag":
                    bad[L + rng.randrange(16)] ^= 4
                elif kind == "nonce":
                    bad[L + 16 + rng.randrange(12)] ^= 2
                elif kind == "aad_short":
                    bad_aad = bad_aad[:-1]
                elif kind == "aad_long":
                    bad_aad = bad_aad + b"\0"
                ref = bytearray(bad)
                want_n = O.aesgo_decrypt(key, ref, bytes(bad_aad))
                assert want_n < 0, (a, L, kind)  # the oracle refuses every one of them
                tail = bytes(bad[L:])
                n, err = aes.Decrypt(bad, bytes(bad_aad))
                if err is None or bytes(bad[:L]) != bytes(L) or bytes(bad[L:]) != tail:
                    errs.append((a, L, kind))
            n, err = aes.Decrypt(data, aad)  # untouched, it still opens
            if err is not None or bytes(data[:L]) != pt:
                errs.append((a, L, "intact"))
    assert not errs, errs


def test_stale_tail(ctx):
    """One thread, so the resident slot is reused: 1000 B of 0xFF additional data, then 5 B and 17 B
    whose last blocks lie over those bytes."""
    from quantum_amd.crypto import AES

    key = bytes(range(71, 103))
    aes = AES(key, ctx=ctx)
    rng = random.Random(0xA008)
    for L in (100, 1350):
        assert pair(aes, key, L, b"\xff" * 1000, rng) is None
        assert pair(aes, key, L, rng.randbytes(5), rng) is None
        assert pair(aes, key, L, b"\xff" * 1000, rng) is None
        assert pair(aes, key, L, rng.randbytes(17), rng) is None


def test_threads(ctx):
    from quantum_amd.crypto import AES

    key = bytes(range(81, 113))
    aes = AES(key, ctx=ctx)
    errs = []

    def work(t):
        rng = random.Random(0xA100 + t)
        for i in range(30):
            a = (0, 4, 5, 13, 64, 1000)[(i + t) % 6]
            L = rng.choice([0, 5, 16, 31, 100, 1350, rng.randrange(0, 4000)])
            e = pair(aes, key, L, rng.randbytes(a), rng)
            if e:
                errs.append((t, e))
                return

    ths = [threading.Thread(target=work, args=(t,)) for t in range(8)]
    for th in ths:
        th.start()
    for th in ths:
        th.join()
    assert not errs, errs[:5]
    assert ctx.resident_stats()["broken"] == 0
