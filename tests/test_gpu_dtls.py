"""GPU: qgcm_dtls_seal / qgcm_dtls_open (gcm_dtls_kernel in quantum_amd/csrc/gcm_kernels.hip, the numbering and
window launches of dtls_kernels.hip) against the Python model of tests/dtls_model.py, byte for byte: arena,
header entries, lengths, status, reason and session state.

A wave tile is 16 packets of one key, a scan tile 256 positions: the batch sizes sit around both, the lengths
around the 16-byte block, the dword (L % 4 decides how the tag is stored) and block 254, where the counter's
second byte changes."""
import json
import os

import numpy as np
import pytest

import dtls_model as M
from conftest import GOLDEN
from quantum_amd import dtls

pytestmark = pytest.mark.gpu

MAX_KEYS = 300          # sessions 0..127 own key slots 2p, 2p + 1; slots 290.. are the other calls'
SHORT, LONG = 1536, 16448
LONG_LENS = [4063, 4064, 4065, 4080, 4081, 8191, 16383, 16384]


@pytest.fixture(scope="module")
def cx():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from quantum_amd.crypto import Context

    old = os.environ.get("QGCM_FLAT_GHASH_KEYS")
    os.environ["QGCM_FLAT_GHASH_KEYS"] = "0"  # the per-packet GHASH tables are not used here
    try:
        c = Context(device=0, max_keys=MAX_KEYS)
    finally:
        if old is None:
            del os.environ["QGCM_FLAT_GHASH_KEYS"]
        else:
            os.environ["QGCM_FLAT_GHASH_KEYS"] = old
    yield c
    c.close()


def install(ctx, model: dict, first: int = 0):
    """Model sessions p -> context sessions first + p (key slots 2 (first + p), + 1), fresh windows."""
    ps = sorted(model)
    assert ps == list(range(len(ps)))
    dtls.sessions_set(ctx, first, [
        dtls.Session(s.write_key, s.read_key, s.write_iv, s.read_iv, 2 * (first + p), 2 * (first + p) + 1,
                     s.write_epoch, s.read_epoch, s.write_seq) for p, s in ((p, model[p]) for p in ps)])
    for s in model.values():
        s.R = s.W = 0


def run(ctx, seal: bool, arena, lens, peer, hdr, first: int = 0):
    """One device call on copies of the host arrays -> (arena, lens, hdr, status, reason) as numpy."""
    import torch

    n, stride = arena.shape
    d_arena = torch.from_numpy(arena.reshape(-1).copy()).cuda()
    d_lens = torch.from_numpy(lens.astype(np.uint32).view(np.int32).copy()).cuda()
    dev_peer = np.where(peer == M.NO_PEER, M.NO_PEER, peer.astype(np.uint64) + first).astype(np.uint32)
    d_peer = torch.from_numpy(dev_peer.view(np.int32).copy()).cuda()
    d_hdr = torch.from_numpy(hdr.reshape(-1).copy()).cuda()
    d_status = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    d_reason = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    (dtls.seal if seal else dtls.open)(ctx, d_arena, stride, n, d_lens, d_peer, d_hdr, d_status, d_reason)
    torch.cuda.synchronize()
    return (d_arena.cpu().numpy().reshape(n, stride), d_lens.cpu().numpy().view(np.uint32),
            d_hdr.cpu().numpy().reshape(n, 32), d_status.cpu().numpy(), d_reason.cpu().numpy())


def check(ctx, seal: bool, model: dict, arena, lens, peer, hdr, first: int = 0, what=""):
    """Device against model on the same inputs; returns the model's outputs (the next call's inputs)."""
    got = run(ctx, seal, arena, lens, peer, hdr, first)
    w_arena, w_lens, w_hdr = arena.copy(), lens.astype(np.uint32).copy(), hdr.copy()
    w_status, w_reason = (M.seal_batch if seal else M.open_batch)(model, w_arena, w_lens, peer, w_hdr)
    assert got[3].tolist() == w_status.tolist(), what
    assert got[4].tolist() == w_reason.tolist(), what
    assert got[1].tolist() == w_lens.tolist(), what
    assert np.array_equal(got[2], w_hdr), what
    bad = np.flatnonzero((got[0] != w_arena).any(axis=1))
    assert bad.size == 0, f"{what}: slots {bad[:8].tolist()} differ (lens {lens[bad[:8]].tolist()})"
    for p, s in model.items():
        st = dtls.session_state(ctx, first + p)
        assert st == s.state(), f"{what}: session {p}"
    return w_arena, w_lens, w_hdr, w_status, w_reason


def plain_batch(rng, n: int, stride: int, lens, sessions: int):
    """Random slots (payload and the sentinel bytes behind it alike), 0xA5 header entries, interleaved sessions."""
    arena = rng.integers(0, 256, (n, stride), dtype=np.uint8)
    peer = ((np.arange(n) * 7 + 3) % sessions).astype(np.uint32)
    return arena, np.asarray(lens, np.uint32), peer, np.full((n, 32), 0xA5, np.uint8)


@pytest.mark.parametrize("sessions", [1, 3, 64])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 63, 64, 65, 300])
def test_seal_short(cx, sessions, n):
    rng = np.random.default_rng(0xD7150100 + 1000 * sessions + n)
    model = M.make_sessions(sessions, 0xD715 + sessions)
    install(cx, model)
    lens = [1 + (i * 11 + n) % 48 for i in range(n)]
    batch = plain_batch(rng, n, SHORT, lens, sessions)
    check(cx, True, model, *batch, what="first call")
    # a second call continues each session's numbering
    lens2 = [1 + (i * 5 + 7) % 48 for i in range(n)]
    check(cx, True, model, *plain_batch(rng, n, SHORT, lens2, sessions), what="second call")
    assert sum(s.write_seq for s in model.values()) == 2 * n


def test_seal_every_short_length_and_single_packet_sessions(cx):
    """Lengths 1..48 once each, and 48 sessions with one packet each."""
    rng = np.random.default_rng(0xD7150200)
    model = M.make_sessions(64, 0xD7152)
    install(cx, model)
    arena, lens, _, hdr = plain_batch(rng, 48, SHORT, list(range(1, 49)), 64)
    peer = rng.permutation(64)[:48].astype(np.uint32)
    check(cx, True, model, arena, lens, peer, hdr)
    assert sorted(s.write_seq for s in model.values()) == [0] * 16 + [1] * 48


@pytest.mark.parametrize("sessions", [1, 3])
def test_seal_long(cx, sessions):
    rng = np.random.default_rng(0xD7150300 + sessions)
    model = M.make_sessions(sessions, 0xD7153 + sessions)
    install(cx, model)
    lens = LONG_LENS + [4081, 1, 4064, 47, 16384, 4063, 17, 8191, 4080]  # 17 packets: a full tile and one more
    check(cx, True, model, *plain_batch(rng, len(lens), LONG, lens, sessions))


def test_seal_rejects(cx):
    rng = np.random.default_rng(0xD7150400)
    model = M.make_sessions(5, 0xD7154)
    install(cx, model)
    dtls.sessions_clear(cx, 3, 1)       # an unset session
    del model[3]
    cx.clear_keys(2 * 4, 1)             # session 4 keeps its entry but its write key slot is cleared
    model[4].write_key_ok = False
    peer = np.array([0, 1, 0, 2, M.NO_PEER, 1, 3, 4, 0, 250, 2, 2, 1, 0, 299, 300], np.uint32)
    lens = np.array([1, 16, 17, 0, 40, 16384, 40, 40, 16385, 40, SHORT - 16, SHORT - 15, 33, 48, 40, 40], np.uint32)
    arena = rng.integers(0, 256, (len(lens), SHORT), dtype=np.uint8)
    hdr = np.full((len(lens), 32), 0xA5, np.uint8)
    out = check(cx, True, {p: s for p, s in model.items() if p != 4}, arena, lens, peer, hdr)
    assert out[4].tolist() == [0, 0, 0, M.MALFORMED, M.NO_SESSION, M.MALFORMED, M.NO_SESSION, M.NO_SESSION,
                               M.MALFORMED, M.NO_SESSION, 0, M.MALFORMED, 0, 0, M.NO_SESSION, M.NO_SESSION]
    # stride: L + 16 > stride at the stride itself
    model = M.make_sessions(1, 0xD7155)
    install(cx, model)
    lens = np.array([48, 49, 64, 33], np.uint32)
    arena = rng.integers(0, 256, (4, 64), dtype=np.uint8)
    out = check(cx, True, model, arena, lens, np.zeros(4, np.uint32), np.full((4, 32), 0xA5, np.uint8))
    assert out[3].tolist() == [1, 0, 0, 1]


def test_seal_sequence_exhausted(cx):
    rng = np.random.default_rng(0xD7150500)
    model = M.make_sessions(2, 0xD7156, write_seq=M.SEQ_END - 3)
    model[1].write_seq = 7
    install(cx, model)
    peer = np.array([0, 0, 0, 1, 0, 0, 0], np.uint32)
    lens = np.array([10, 11, 0, 12, 13, 14, 15], np.uint32)  # the rejected one in between takes no number
    arena = rng.integers(0, 256, (7, SHORT), dtype=np.uint8)
    out = check(cx, True, model, arena, lens, peer, np.full((7, 32), 0xA5, np.uint8))
    assert out[3].tolist() == [1, 1, 0, 1, 1, 0, 0]
    assert out[4].tolist() == [0, 0, M.MALFORMED, 0, 0, M.SEQ_EXHAUSTED, M.SEQ_EXHAUSTED]
    assert model[0].write_seq == M.SEQ_END
    # saturated: nothing more is sealed
    out = check(cx, True, model, arena[:2], lens[:2], peer[:2], np.full((2, 32), 0xA5, np.uint8))
    assert out[4].tolist() == [M.SEQ_EXHAUSTED] * 2


def records(rx: dict, stride: int, items, rng):
    """Slots and header entries holding records for the receiving sessions `rx`: items = (session, seq, L,
    authentic); a record that is not authentic has a tag bit flipped."""
    n = len(items)
    arena = rng.integers(0, 256, (n, stride), dtype=np.uint8)
    hdr = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    lens, peer = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    for i, (p, seq, L, auth) in enumerate(items):
        s = rx[p]
        h = M.header(s.read_epoch, seq, L)
        body = bytearray(M.seal_record(s.read_key, s.read_iv, h, arena[i, :L].tobytes()))
        if not auth:
            body[L + (i % 16)] ^= 1 << (i % 8)
        arena[i, :L + 16] = np.frombuffer(bytes(body), np.uint8)
        hdr[i, :21] = np.frombuffer(h, np.uint8)
        lens[i], peer[i] = L + 16, p
    return arena, lens, peer, hdr


def flipped(rx: dict, stride: int, L: int, bits, rng):
    """One L-byte record per listed bit of its 21 + L + 16 bytes, each copy with that bit flipped and a sequence
    number of its own."""
    arena, lens, peer, hdr = records(rx, stride, [(0, 1 + k, L, True) for k in range(len(bits))], rng)
    for k, bit in enumerate(bits):
        byte, m = bit >> 3, 0x80 >> (bit & 7)
        if byte < 21:
            hdr[k, byte] ^= m
        else:
            arena[k, byte - 21] ^= m
    return arena, lens, peer, hdr


def test_open_forgeries_every_bit(cx):
    rng = np.random.default_rng(0xD7150600)
    rx = M.make_sessions(1, 0xD7157)
    install(cx, rx)
    batch = flipped(rx, SHORT, 33, list(range(8 * (21 + 33 + 16))), rng)
    assert len(batch[1]) == 560
    out = check(cx, False, rx, *batch)
    assert out[3].sum() == 0 and rx[0].R == 0 and rx[0].W == 0  # nothing delivered, the window untouched
    reason = out[4]
    assert set(reason[:8].tolist()) == {M.NOT_APPDATA}                        # type
    assert set(reason[8:40].tolist()) == {M.MALFORMED}                        # version, epoch
    assert set(reason[40:88].tolist()) == {M.AUTH}                            # sequence number
    assert set(reason[88:104].tolist()) == {M.MALFORMED}                      # length
    assert set(reason[104:].tolist()) == {M.AUTH}                             # nonce, ciphertext, tag
    auth = np.flatnonzero(reason == M.AUTH)
    assert not out[0][auth, :33].any()                                        # the would-be plaintext zeroed
    # the session still takes the authentic records afterwards
    check(cx, False, rx, *records(rx, SHORT, [(0, 5, 33, True), (0, 5, 33, True)], rng))
    assert (rx[0].R, rx[0].W) == (5, 1)


def test_open_forgeries_long_record(cx):
    rng = np.random.default_rng(0xD7150700)
    rx = M.make_sessions(1, 0xD7158)
    install(cx, rx)
    L = 4081
    bits = list(range(8 * 21)) + list(range(8 * 21, 8 * (21 + 16))) + \
        list(range(8 * (21 + L - 16), 8 * (21 + L))) + list(range(8 * (21 + L), 8 * (21 + L + 16)))
    out = check(cx, False, rx, *flipped(rx, LONG, L, bits, rng))
    assert out[3].sum() == 0 and rx[0].R == 0 and rx[0].W == 0


def window_state_batch(R0: int, W0: int):
    """Numbers that bring a fresh window to (R0, W0) (W0 has bit 0 set), in ascending order."""
    return [R0 - k for k in range(63, -1, -1) if (W0 >> k) & 1 and R0 - k >= 0]


@pytest.mark.parametrize("case", M.window_cases(), ids=lambda c: c[0])
def test_open_window_cases(cx, case):
    _, R0, W0, pkts = case
    rng = np.random.default_rng(0xD7150800 + R0)
    rx = M.make_sessions(2, 0xD7159)
    install(cx, rx)
    if R0 or W0:
        first = window_state_batch(R0, W0)
        check(cx, False, rx, *records(rx, SHORT, [(1, s, 20, True) for s in first], rng), what="state")
        assert (rx[1].R, rx[1].W) == (R0, W0)
    # session 0 carries a few packets of its own in between
    items = []
    for k, (s, a) in enumerate(pkts):
        items.append((1, s, 17 + k % 30, bool(a)))
        if k % 3 == 0:
            items.append((0, 1000 + k, 40, True))
    check(cx, False, rx, *records(rx, SHORT, items, rng), what="case")


def test_open_window_large_and_interleaved(cx):
    """2000 packets of one session, numbers 1..2000 shuffled within blocks of 32 (eight scan tiles), with every
    seventh packet a second copy; then eight sessions interleaved over three calls that carry the state."""
    rng = np.random.default_rng(0xD7150900)
    rx = M.make_sessions(8, 0xD715A)
    install(cx, rx)
    seqs = np.arange(1, 2001)
    for b in range(0, 2000, 32):
        rng.shuffle(seqs[b:b + 32])
    items = []
    for k, s in enumerate(seqs.tolist()):
        items.append((0, s, 1 + k % 40, True))
        if k % 7 == 0:
            items.append((0, int(seqs[max(0, k - 20)]), 24, True))
    out = check(cx, False, rx, *records(rx, 64, items, rng), what="one session")
    assert out[3].sum() == 2000 and rx[0].R == 2000
    base = 0
    for call in range(3):
        items = []
        for k in range(400):
            p = int(rng.integers(0, 8))
            s = max(0, base + int(rng.integers(-70, 90)))
            items.append((p, s, 16 + k % 33, rng.random() < 0.9))
        base += 60
        check(cx, False, rx, *records(rx, 64, items, rng), what=f"call {call}")


def test_open_rejects(cx):
    """NO_SESSION, epoch, version, length field, short and long B, B > stride -- by the model's precedence."""
    rng = np.random.default_rng(0xD7150A00)
    rx = M.make_sessions(3, 0xD715B)
    install(cx, rx)
    dtls.sessions_clear(cx, 2, 1)
    del rx[2]
    arena, lens, peer, hdr = records({0: rx[0], 1: rx[1], 2: M.make_sessions(1, 1)[0]}, SHORT,
                                     [(k % 3, 1 + k, 24, True) for k in range(12)], rng)
    peer[9] = M.NO_PEER
    hdr[0, 3:5] = (0, 2)             # another epoch
    hdr[1, 1] = 0xFF                 # another version
    hdr[3, 12] ^= 1                  # length field
    lens[4] = 16                     # no payload
    hdr[4, 11:13] = (0, 24)
    lens[6] = SHORT + 4              # past the stride
    hdr[6, 11:13] = np.frombuffer((8 + SHORT + 4).to_bytes(2, "big"), np.uint8)
    hdr[7, 0] = 22                   # handshake record with a bad epoch too: NOT_APPDATA wins
    hdr[7, 3:5] = (0, 9)
    out = check(cx, False, rx, arena, lens, peer, hdr)
    assert out[4].tolist() == [M.MALFORMED, M.MALFORMED, M.NO_SESSION, M.MALFORMED, M.MALFORMED, M.NO_SESSION,
                               M.MALFORMED, M.NOT_APPDATA, M.NO_SESSION, M.NO_SESSION, 0, M.NO_SESSION]


def test_open_golden_openssl_records(cx):
    """Records OpenSSL wrote (tests/golden/dtls_records.json), without libssl: all delivered with the fixture's
    plaintext; fed again, all REPLAY."""
    path = os.path.join(GOLDEN, "dtls_records.json")
    g = json.load(open(path))
    rng = np.random.default_rng(0xD7150B00)
    kb = bytes.fromhex(g["key_block"])
    ep = g["epoch"]
    # session 0 is the server's view (it reads what the client wrote), session 1 the client's
    rx = {0: M.Session(kb[32:64], kb[0:32], kb[68:72], kb[64:68], ep, ep),
          1: M.Session(kb[0:32], kb[32:64], kb[64:68], kb[68:72], ep, ep)}
    install(cx, rx)
    items = [(0, r) for r in g["client_records"]] + [(1, r) for r in g["server_records"] + g["model_records"]]
    n, stride = len(items), LONG
    arena = rng.integers(0, 256, (n, stride), dtype=np.uint8)
    hdr = np.zeros((n, 32), np.uint8)
    lens, peer = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    for i, (p, r) in enumerate(items):
        rec = bytes.fromhex(r["record"])
        hdr[i, :21] = np.frombuffer(rec[:21], np.uint8)
        arena[i, :len(rec) - 21] = np.frombuffer(rec[21:], np.uint8)
        lens[i], peer[i] = len(rec) - 21, p
    out = check(cx, False, rx, arena, lens, peer, hdr)
    assert out[3].tolist() == [1] * n
    for i, (_, r) in enumerate(items):
        pt = bytes.fromhex(r["plaintext"])
        assert out[1][i] == len(pt) and out[0][i, :len(pt)].tobytes() == pt
    out = check(cx, False, rx, arena, lens, peer, hdr)
    assert out[4].tolist() == [M.REPLAY] * n


@pytest.mark.parametrize("sessions,n,stride", [(1, 17, SHORT), (3, 65, SHORT), (64, 300, SHORT), (3, 17, LONG)])
def test_round_trip(cx, sessions, n, stride):
    """Sealed on the device, opened on the device under the mirrored sessions (context sessions 64 + p)."""
    rng = np.random.default_rng(0xD7150C00 + n)
    tx = M.make_sessions(sessions, 0xD715C + sessions)
    rx = M.mirror(tx)
    install(cx, tx)
    install(cx, rx, first=64)
    lens = [1 + (i * 13) % 48 for i in range(n)] if stride == SHORT else (LONG_LENS * 3)[:n]
    arena, lens, peer, hdr = plain_batch(rng, n, stride, lens, sessions)
    s_arena, s_lens, s_hdr, s_status, _ = check(cx, True, tx, arena, lens, peer, hdr)
    assert s_status.all()
    o_arena, o_lens, _, o_status, _ = check(cx, False, rx, s_arena, s_lens, peer, s_hdr, first=64)
    assert o_status.all() and o_lens.tolist() == lens.tolist()
    for i in range(n):
        assert np.array_equal(o_arena[i, :lens[i]], arena[i, :lens[i]])


def test_round_trip_every_length_to_130(cx):
    """Lengths 1..130 once each over three sessions, sealed, then opened under the mirrored sessions: every
    L mod 64 twice -- the lane that owns the partial block, the lane that computes E_K(J0), the words of the
    partial block and the shifts of dtls_write_tag in every combination (the other tests reach 49..63,
    65..79 and so on only through four long records)."""
    rng = np.random.default_rng(0xD7150E00)
    tx = M.make_sessions(3, 0xD715E)
    rx = M.mirror(tx)
    install(cx, tx)
    install(cx, rx, first=64)
    arena, lens, peer, hdr = plain_batch(rng, 130, SHORT, list(range(1, 131)), 3)
    s_arena, s_lens, s_hdr, s_status, _ = check(cx, True, tx, arena, lens, peer, hdr, what="seal")
    assert s_status.all()
    o_arena, o_lens, _, o_status, _ = check(cx, False, rx, s_arena, s_lens, peer, s_hdr, first=64, what="open")
    assert o_status.all() and o_lens.tolist() == lens.tolist()
    for i in range(130):
        assert np.array_equal(o_arena[i, :lens[i]], arena[i, :lens[i]])


def test_existing_batch_calls_unaffected(cx):
    """After DTLS traffic a keyed qgcm_seal_batch / qgcm_open_batch on other key slots gives the oracle's bytes."""
    import torch

    from oracle import oracle as O
    from quantum_amd import batch

    rng = np.random.default_rng(0xD7150D00)
    model = M.make_sessions(3, 0xD715D)
    install(cx, model)
    check(cx, True, model, *plain_batch(rng, 65, SHORT, [1 + i % 48 for i in range(65)], 3))
    keys = rng.integers(0, 256, 64, dtype=np.uint8).tobytes()
    cx.set_keys(290, keys)
    n, stride = 40, 256
    klens = (1 + (np.arange(n) * 7) % 200).astype(np.uint32)
    kidx = (np.arange(n) % 2).astype(np.uint32)
    offs = (np.arange(n, dtype=np.uint64) * stride)
    arena = rng.integers(0, 256, n * stride, dtype=np.uint8)
    nonces = rng.integers(0, 256, 12 * n, dtype=np.uint8)
    want = arena.copy()
    O.aesgo_seal_descs(keys, want, offs, klens, kidx, nonces, 4)
    d_arena = torch.from_numpy(arena.copy()).cuda()
    status = torch.zeros(n, dtype=torch.uint8, device="cuda")
    batch.seal_batch(cx, d_arena, batch.make_descs(offs, klens, kidx + 290, "cuda"), n,
                     torch.from_numpy(nonces).cuda(), status=status)
    torch.cuda.synchronize()
    assert np.array_equal(d_arena.cpu().numpy(), want) and int(status.sum()) == n
    batch.open_batch(cx, d_arena, batch.make_descs(offs, klens + 28, kidx + 290, "cuda"), n, status=status)
    torch.cuda.synchronize()
    back = d_arena.cpu().numpy().reshape(n, stride)
    assert int(status.sum()) == n
    for i in range(n):
        assert np.array_equal(back[i, :4 + klens[i]], arena.reshape(n, stride)[i, :4 + klens[i]])
