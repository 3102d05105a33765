"""CPU: the DTLS record layer's framing, key block and window against OpenSSL itself -- an in-process DTLS 1.2
session (tests/cpp_dtls/ossl_dtls_peer.c, a child process over an AF_UNIX socketpair, no network).
qgcm_dtls_key_block and the model's PRF give OpenSSL's keys; the model opens the records OpenSSL writes, in both
directions; OpenSSL's SSL_read returns the plaintext of records the model seals; a replayed record is dropped by
both.  Skips only where libssl is absent."""
import numpy as np
import pytest

import dtls_model as M
import dtls_peer
from quantum_amd import dtls

LENGTHS = (1, 15, 16, 17, 33, 1350, 4081)

pytestmark = pytest.mark.skipif(not dtls_peer.available(), reason="libssl is not installed")


@pytest.fixture(scope="module")
def peer(tmp_path_factory):
    p = dtls_peer.Peer(dtls_peer.build(str(tmp_path_factory.mktemp("dtls_peer"))))
    yield p
    p.close()


def sides(block: bytes):
    """(write key, write IV) of client and server from the 72-byte key block."""
    return {"c": (block[0:32], block[64:68]), "s": (block[32:64], block[68:72])}


def test_key_block_is_openssls(peer):
    assert peer.cipher == "ECDHE-ECDSA-AES256-GCM-SHA384"
    block = dtls.key_block(peer.master, peer.client_random, peer.server_random)
    assert block == M.key_block(peer.master, peer.client_random, peer.server_random)
    # the keys are right when they open what OpenSSL wrote
    rec = peer.write("c", b"key check")
    key, iv = sides(block)["c"]
    assert M.open_record(key, iv, rec[:21], rec[21:]) == b"key check"
    wrong, _ = sides(block)["s"]
    assert M.open_record(wrong, iv, rec[:21], rec[21:]) is None


@pytest.mark.parametrize("side", ["c", "s"])
def test_model_opens_openssl_records(peer, side):
    block = M.key_block(peer.master, peer.client_random, peer.server_random)
    key, iv = sides(block)[side]
    rng = np.random.default_rng(0xD7150E00)
    seqs = []
    for L in LENGTHS:
        pt = rng.integers(0, 256, L, dtype=np.uint8).tobytes()
        rec = peer.write(side, pt)
        assert rec[0] == 23 and rec[1:3] == b"\xfe\xfd" and rec[3:5] == b"\x00\x01"
        assert int.from_bytes(rec[11:13], "big") == 8 + L + 16 == len(rec) - 13
        assert M.open_record(key, iv, rec[:21], rec[21:]) == pt
        seqs.append(int.from_bytes(rec[5:11], "big"))
    assert seqs == list(range(seqs[0], seqs[0] + len(LENGTHS)))  # one record per write, numbered in order


@pytest.mark.parametrize("writer,reader", [("c", "s"), ("s", "c")])
def test_openssl_reads_model_records_and_drops_replays(peer, writer, reader):
    block = M.key_block(peer.master, peer.client_random, peer.server_random)
    key, iv = sides(block)[writer]
    rng = np.random.default_rng(0xD7150F00)
    seq = 1000
    for L in LENGTHS:
        pt = rng.integers(0, 256, L, dtype=np.uint8).tobytes()
        h = M.header(1, seq, L)  # explicit nonce = epoch | seq (RFC 5288 3)
        rec = h + M.seal_record(key, iv, h, pt)
        peer.inject(reader, rec)
        assert peer.read(reader) == pt
        peer.inject(reader, rec)  # the same record again: dropped silently
        assert peer.read(reader) is None
        # ... and by the model's window, in the state OpenSSL's is in
        ok1, R, W = M.window_step(seq - 1, 1, seq)
        ok2, _, _ = M.window_step(R, W, seq)
        assert ok1 and not ok2
        seq += 1
    # a forged record (one tag bit) is dropped too, and does not block the authentic one that follows
    h = M.header(1, seq, 33)
    pt = bytes(range(33))
    rec = bytearray(h + M.seal_record(key, iv, h, pt))
    rec[-1] ^= 1
    peer.inject(reader, bytes(rec))
    assert peer.read(reader) is None
    rec[-1] ^= 1
    peer.inject(reader, bytes(rec))
    assert peer.read(reader) == pt
