"""CPU: the host forms of the DTLS record layer's ordered rules (qgcm_dtls_number_cpu, qgcm_dtls_replay_cpu:
quantum_amd/csrc/dtls_core.h) against the Python model of tests/dtls_model.py, the parallel form of the
anti-replay window against the packet-by-packet one, qgcm_dtls_key_block against the model's PRF, and the
argument errors of the new calls.  No GPU."""
import ctypes as C
import time

import numpy as np
import pytest

import dtls_model as M
from quantum_amd import _lib, dtls

STRIDE = 1536


def lib_sessions(model: dict, n_sessions: int):
    """dtls.Session list 0..n_sessions-1 (slots 2p, 2p+1) and the `set` flags for a model's sessions."""
    out, is_set = [], np.zeros(n_sessions, np.uint8)
    for p in range(n_sessions):
        s = model.get(p)
        if s is None or not s.write_key_ok:
            out.append(dtls.Session(bytes(32), bytes(32), bytes(4), bytes(4), 2 * p, 2 * p + 1))
            continue
        is_set[p] = 1
        out.append(dtls.Session(s.write_key, s.read_key, s.write_iv, s.read_iv, 2 * p, 2 * p + 1, s.write_epoch,
                                s.read_epoch, s.write_seq))
    return out, is_set


def check_number(model: dict, n_sessions: int, lens, peer, stride=STRIDE):
    lens = np.asarray(lens, np.uint32)
    peer = np.asarray(peer, np.uint32)
    sess, is_set = lib_sessions(model, n_sessions)
    wseq = np.array([s.write_seq for s in sess], np.uint64)
    got_lens = lens.copy()
    hdr, status, reason = dtls.number_cpu(sess, is_set, wseq, stride, got_lens, peer)
    want_lens, want_hdr = lens.copy(), np.full((len(lens), 32), 0xEE, np.uint8)
    wstatus, wreason = M.number_batch(model, stride, want_lens, peer, want_hdr)
    assert status.tolist() == wstatus.tolist()
    assert reason.tolist() == wreason.tolist()
    assert got_lens.tolist() == want_lens.tolist()
    assert np.array_equal(hdr, want_hdr)  # rejected entries untouched (0xEE) in both
    for p, s in model.items():
        if p < n_sessions and s.write_key_ok:
            assert int(wseq[p]) == s.write_seq, p
    return status, reason


def test_number_interleaved_sessions_and_rejects():
    model = M.make_sessions(5, 0xD715)
    del model[3]                       # an unset session
    model[4].write_key_ok = False      # a cleared key slot
    peer = [0, 1, 0, 2, M.NO_PEER, 1, 3, 4, 0, 9, 2, 2, 1, 0]
    lens = [1, 16, 17, 0, 40, 16384, 40, 40, 16385, 40, STRIDE - 16, STRIDE - 15, 33, 48]
    status, reason = check_number(model, 6, lens, peer)
    assert reason.tolist() == [0, 0, 0, M.MALFORMED, M.NO_SESSION, M.MALFORMED, M.NO_SESSION, M.NO_SESSION,
                               M.MALFORMED, M.NO_SESSION, 0, M.MALFORMED, 0, 0]
    # a second call continues the numbering
    check_number(model, 6, [5, 6, 7], [0, 0, 1])
    assert model[0].write_seq == 5 and model[1].write_seq == 3 and model[2].write_seq == 1


def test_number_header_bytes():
    model = {0: M.Session(bytes(32), bytes(32), bytes(4), bytes(4), write_epoch=0x0102, write_seq=0x0A0B0C0D0E0F)}
    sess, is_set = lib_sessions(model, 1)
    wseq = np.array([0x0A0B0C0D0E0F], np.uint64)
    lens = np.array([1350], np.uint32)
    hdr, status, reason = dtls.number_cpu(sess, is_set, wseq, STRIDE, lens, np.array([0], np.uint32))
    want = bytes([23, 0xFE, 0xFD, 1, 2, 0x0A, 0x0B, 0x0C, 0x0D, 0x0E, 0x0F]) + (8 + 1350 + 16).to_bytes(2, "big") + \
        bytes([1, 2, 0x0A, 0x0B, 0x0C, 0x0D, 0x0E, 0x0F]) + bytes(11)
    assert hdr[0].tobytes() == want and lens[0] == 1366 and status[0] == 1 and reason[0] == 0
    assert M.additional_data(want, 1350) == bytes([1, 2, 0x0A, 0x0B, 0x0C, 0x0D, 0x0E, 0x0F, 23, 0xFE, 0xFD]) + \
        (1350).to_bytes(2, "big")


def test_number_sequence_exhausted_saturates():
    model = M.make_sessions(2, 0xD716, write_seq=M.SEQ_END - 3)
    model[1].write_seq = 7
    # session 0: a rejected packet between the numbered ones takes no number; three sealed, two exhausted
    status, reason = check_number(model, 2, [10, 10, 0, 10, 10, 10, 10], [0, 0, 0, 1, 0, 0, 0])
    assert status.tolist() == [1, 1, 0, 1, 1, 0, 0]
    assert reason.tolist() == [0, 0, M.MALFORMED, 0, 0, M.SEQ_EXHAUSTED, M.SEQ_EXHAUSTED]
    assert model[0].write_seq == M.SEQ_END and model[1].write_seq == 8


@pytest.mark.parametrize("case", M.window_cases(), ids=lambda c: c[0])
def test_replay_cases(case):
    _, R0, W0, pkts = case
    seq = np.array([s for s, _ in pkts], np.uint64)
    auth = np.array([a for _, a in pkts], np.uint8)
    sess = np.zeros(len(pkts), np.uint32)
    want_state = np.array([[R0, W0]], np.uint64)
    want = M.replay_batch(sess, seq, auth, want_state)
    for parallel in (False, True):
        state = np.array([[R0, W0]], np.uint64)
        got = dtls.replay_cpu(sess, seq, auth, state, parallel)
        assert got.tolist() == want.tolist(), parallel
        assert state.tolist() == want_state.tolist(), parallel


def test_replay_edge_is_63_not_64():
    state = np.array([[100, 1]], np.uint64)
    got = dtls.replay_cpu([0, 0], [37, 36], [1, 1], state, True)
    assert got.tolist() == [1, 0] and state.tolist() == [[100, 1 | (1 << 63)]]


def test_replay_parallel_equals_sequential_random():
    """Seeded random batches, several sessions interleaved, numbers clustered around the window's edges, forged
    packets mixed in, state carried from batch to batch.  Bounded to a few seconds."""
    rng = np.random.default_rng(0xD7150001)
    t0, rounds = time.monotonic(), 0
    while rounds < 400 and time.monotonic() - t0 < 3.0:
        ns = int(rng.integers(1, 6))
        state_m = np.zeros((ns, 2), np.uint64)
        state_m[:, 0] = rng.integers(0, 300, ns)
        state_m[:, 1] = rng.integers(0, 2 ** 63, ns, dtype=np.uint64) * 2 + rng.integers(0, 2, ns).astype(np.uint64)
        state_s, state_p = state_m.copy(), state_m.copy()
        for _ in range(3):
            n = int(rng.integers(0, 120))
            sess = rng.integers(0, ns + 1, n).astype(np.uint32)  # ns itself: a session out of range
            base = state_m[np.minimum(sess, ns - 1), 0].astype(np.int64)
            seq = np.maximum(0, base + rng.integers(-70, 70, n)).astype(np.uint64)
            far = rng.random(n) < 0.05
            seq[far] += rng.integers(60, 400, int(far.sum())).astype(np.uint64)
            auth = (rng.random(n) < 0.8).astype(np.uint8)
            want = M.replay_batch(sess, seq, auth, state_m)
            got_s = dtls.replay_cpu(sess, seq, auth, state_s, False)
            got_p = dtls.replay_cpu(sess, seq, auth, state_p, True)
            assert got_s.tolist() == want.tolist()
            assert got_p.tolist() == want.tolist()
            assert state_s.tolist() == state_m.tolist() and state_p.tolist() == state_m.tolist()
        rounds += 1
    assert rounds >= 20


def test_key_block_matches_prf():
    rng = np.random.default_rng(0xD7150002)
    for _ in range(4):
        master, cr, sr = (rng.integers(0, 256, k, dtype=np.uint8).tobytes() for k in (48, 32, 32))
        assert dtls.key_block(master, cr, sr) == M.key_block(master, cr, sr)
    # RFC 5246 5: A(1) = HMAC(secret, seed), first block HMAC(secret, A(1) | seed) -- an all-zero vector by hand
    import hashlib
    import hmac

    seed = b"key expansion" + bytes(64)
    a1 = hmac.new(bytes(48), seed, hashlib.sha384).digest()
    assert dtls.key_block(bytes(48), bytes(32), bytes(32))[:48] == hmac.new(bytes(48), a1 + seed, hashlib.sha384).digest()


def test_argument_errors():
    L = _lib.lib()
    E_ARG, E_KEY = _lib.QGCM_E_ARG, _lib.QGCM_E_KEY
    buf = C.create_string_buffer(96)
    assert L.qgcm_dtls_key_block(None, buf, buf, buf) == E_ARG
    assert L.qgcm_dtls_key_block(buf, None, buf, buf) == E_ARG
    assert L.qgcm_dtls_key_block(buf, buf, None, buf) == E_ARG
    assert L.qgcm_dtls_key_block(buf, buf, buf, None) == E_ARG
    # the context calls check their context first
    assert L.qgcm_dtls_sessions_set(None, 0, 1, buf) == E_ARG
    assert L.qgcm_dtls_sessions_clear(None, 0, 1) == E_ARG
    assert L.qgcm_dtls_session_state(None, 0, buf) == E_ARG
    assert L.qgcm_dtls_seal(None, buf, 64, 1, buf, buf, buf, buf, None, None) == E_ARG
    assert L.qgcm_dtls_open(None, buf, 64, 1, buf, buf, buf, buf, None, None) == E_ARG
    # number_cpu: missing arrays, a stride that is no multiple of 4 or too short, a write_seq past 2^48
    keys = dtls.keys_array([dtls.Session(bytes(32), bytes(32), bytes(4), bytes(4), 0, 1)])
    wseq = np.zeros(1, np.uint64)
    lens, peer = np.array([8], np.uint32), np.zeros(1, np.uint32)
    hdr, st = np.zeros((1, 32), np.uint8), np.zeros(1, np.uint8)

    def number(k=C.addressof(keys), w=wseq.ctypes.data, stride=64, ln=lens.ctypes.data, p=peer.ctypes.data,
               h=hdr.ctypes.data, s=st.ctypes.data):
        return L.qgcm_dtls_number_cpu(k, None, w, 1, stride, 1, ln, p, h, s, None)

    assert number() == 0 and st[0] == 1
    for kw in ({"k": None}, {"w": None}, {"ln": None}, {"p": None}, {"h": None}, {"s": None}, {"stride": 66},
               {"stride": 16}):
        assert number(**kw) == E_ARG, kw
    wseq[0] = M.SEQ_END + 1
    assert number() == E_ARG
    # replay_cpu: missing arrays, an authentic number past 48 bits
    sess, seq, auth, acc = np.zeros(1, np.uint32), np.array([5], np.uint64), np.ones(1, np.uint8), np.zeros(1, np.uint8)
    state = np.zeros((1, 2), np.uint64)

    def replay(a=sess.ctypes.data, b=seq.ctypes.data, c=auth.ctypes.data, d=state.ctypes.data, e=acc.ctypes.data):
        return L.qgcm_dtls_replay_cpu(1, a, b, c, 1, d, e, 1)

    assert replay() == 0 and acc[0] == 1
    for kw in ({"a": None}, {"b": None}, {"c": None}, {"d": None}, {"e": None}):
        assert replay(**kw) == E_ARG, kw
    seq[0] = M.SEQ_END
    assert replay() == E_ARG
    assert E_KEY == -3
