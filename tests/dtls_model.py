"""A Python model of the DTLS 1.2 record layer on routed batches (include/qgcm.h "DTLS 1.2 records on routed
batches"): record framing, GCM inputs and the key-block PRF from RFC 6347 / RFC 5288 / RFC 5246 with hmac and
hashlib, AES-256-GCM through the oracle (oracle_gcm_seal / oracle_gcm_open take any IV and additional data), the
packet-by-packet anti-replay window of RFC 6347 4.1.2.6, and whole-batch seal and open with every reason code.
It is the yardstick of the CPU and GPU tests; it shares no code with quantum_amd/csrc/dtls_core.h."""
from __future__ import annotations

import hashlib
import hmac
from dataclasses import dataclass

import numpy as np

from oracle import oracle as O

OK, NO_SESSION, NOT_APPDATA, MALFORMED, AUTH, REPLAY, SEQ_EXHAUSTED = range(7)
MAX_PLAIN = 16384
SEQ_END = 1 << 48
NO_PEER = 0xFFFFFFFF
APPDATA = 23
VERSION = b"\xfe\xfd"


def p_sha384(secret: bytes, seed: bytes, n: int) -> bytes:
    """RFC 5246 5: P_hash with HMAC-SHA384."""
    out, a = b"", seed
    while len(out) < n:
        a = hmac.new(secret, a, hashlib.sha384).digest()
        out += hmac.new(secret, a + seed, hashlib.sha384).digest()
    return out[:n]


def key_block(master: bytes, client_random: bytes, server_random: bytes) -> bytes:
    """RFC 5246 6.3 for AES-256-GCM (no MAC keys, 4-byte implicit IVs): 72 bytes."""
    return p_sha384(master, b"key expansion" + server_random + client_random, 72)


def header(epoch: int, seq: int, L: int, explicit: bytes | None = None) -> bytes:
    """The 21 bytes in front of the ciphertext: record header (length = 8 + L + 16), then the explicit nonce
    (epoch | seq, RFC 5288 3, when none is given)."""
    es = epoch.to_bytes(2, "big") + seq.to_bytes(6, "big")
    return bytes([APPDATA]) + VERSION + es + (8 + L + 16).to_bytes(2, "big") + (es if explicit is None else explicit)


def additional_data(h: bytes, L: int) -> bytes:
    """epoch(2) | seq(6) | type | version(2) | L(2), from a header entry."""
    return h[3:11] + h[0:3] + L.to_bytes(2, "big")


def seal_record(key: bytes, iv: bytes, h: bytes, pt: bytes) -> bytes:
    ct, tag = O.gcm_seal(key, iv + h[13:21], additional_data(h, len(pt)), pt)
    return ct + tag


def open_record(key: bytes, iv: bytes, h: bytes, body: bytes) -> bytes | None:
    L = len(body) - 16
    return O.gcm_open(key, iv + h[13:21], additional_data(h, L), body[:L], body[L:])


def window_step(R: int, W: int, s: int) -> tuple[bool, int, int]:
    """RFC 6347 4.1.2.6, one packet: bit k of W means R - k has been seen."""
    if s > R:
        sh = s - R
        return True, s, (((W << sh) | 1) & (2 ** 64 - 1)) if sh < 64 else 1
    d = R - s
    if d >= 64 or (W >> d) & 1:
        return False, R, W
    return True, R, W | (1 << d)


@dataclass
class Session:
    write_key: bytes
    read_key: bytes
    write_iv: bytes
    read_iv: bytes
    write_epoch: int = 1
    read_epoch: int = 1
    write_seq: int = 0
    R: int = 0
    W: int = 0
    write_key_ok: bool = True   # the key slot is set
    read_key_ok: bool = True

    def state(self) -> dict[str, int]:
        return {"write_seq": self.write_seq, "R": self.R, "W": self.W, "set": 1}


def number_batch(sessions: dict, stride: int, lens, peer, hdr):
    """Seal without the crypto: checks, numbers in arena order, header entries, lengths.  Returns (status,
    reason); lens (uint32 array), hdr ([n, 32] uint8) and the sessions' write_seq are updated."""
    n = len(lens)
    status, reason = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    for i in range(n):
        s, L = sessions.get(int(peer[i])), int(lens[i])
        if s is None or not s.write_key_ok:
            reason[i] = NO_SESSION
        elif L == 0 or L > MAX_PLAIN or L + 16 > stride:
            reason[i] = MALFORMED
        elif s.write_seq >= SEQ_END:
            reason[i] = SEQ_EXHAUSTED
        else:
            hdr[i, :21] = np.frombuffer(header(s.write_epoch, s.write_seq, L), np.uint8)
            hdr[i, 21:] = 0
            s.write_seq += 1
            lens[i] = L + 16
            status[i] = 1
    return status, reason


def seal_batch(sessions: dict, arena, lens, peer, hdr):
    """qgcm_dtls_seal on host arrays: arena [n, stride] uint8."""
    before = lens.copy()
    status, reason = number_batch(sessions, arena.shape[1], lens, peer, hdr)
    for i in np.flatnonzero(status):
        s, L = sessions[int(peer[i])], int(before[i])
        body = seal_record(s.write_key, s.write_iv, hdr[i].tobytes(), arena[i, :L].tobytes())
        arena[i, :L + 16] = np.frombuffer(body, np.uint8)
    return status, reason


def open_batch(sessions: dict, arena, lens, peer, hdr):
    """qgcm_dtls_open on host arrays; the sessions' windows advance."""
    n, stride = len(lens), arena.shape[1]
    status, reason = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    for i in range(n):
        s, B, h = sessions.get(int(peer[i])), int(lens[i]), hdr[i].tobytes()
        if s is None or not s.read_key_ok:
            reason[i] = NO_SESSION
        elif h[0] != APPDATA:
            reason[i] = NOT_APPDATA
        elif (h[1:3] != VERSION or int.from_bytes(h[3:5], "big") != s.read_epoch or B < 17 or B > MAX_PLAIN + 16
              or B > stride or int.from_bytes(h[11:13], "big") != 8 + B):
            reason[i] = MALFORMED
        else:
            pt = open_record(s.read_key, s.read_iv, h, arena[i, :B].tobytes())
            if pt is None:
                arena[i, :B - 16] = 0
                reason[i] = AUTH
                continue
            arena[i, :B - 16] = np.frombuffer(pt, np.uint8)
            ok, s.R, s.W = window_step(s.R, s.W, int.from_bytes(h[5:11], "big"))
            if ok:
                lens[i] = B - 16
                status[i] = 1
            else:
                reason[i] = REPLAY
    return status, reason


def replay_batch(session, seq, authentic, state):
    """The window alone over (session, seq, authentic): accept flags; state [n_sessions, 2] = (R, W) updated."""
    accept = np.zeros(len(session), np.uint8)
    for i in range(len(session)):
        p = int(session[i])
        if not authentic[i] or p >= len(state):
            continue
        ok, R, W = window_step(int(state[p, 0]), int(state[p, 1]), int(seq[i]))
        state[p, 0], state[p, 1] = R, W
        accept[i] = 1 if ok else 0
    return accept


def make_sessions(count: int, seed: int, write_seq=0) -> dict:
    """Sessions 0..count-1 with keys from a seeded generator."""
    rng = np.random.default_rng(seed)
    out = {}
    for p in range(count):
        b = rng.integers(0, 256, 72, dtype=np.uint8).tobytes()
        out[p] = Session(b[0:32], b[32:64], b[64:68], b[68:72], 1, 1, write_seq)
    return out


def mirror(sessions: dict) -> dict:
    """The peers' views: each reads what the other writes."""
    return {p: Session(s.read_key, s.write_key, s.read_iv, s.write_iv, s.read_epoch, s.write_epoch)
            for p, s in sessions.items()}


def window_cases():
    """(name, R0, W0, [(seq, authentic)]) for one session: the cases the model decides."""
    full = 2 ** 64 - 1
    return [
        ("in order", 0, 0, [(s, 1) for s in range(1, 40)]),
        ("zero on a fresh session", 0, 0, [(0, 1), (0, 1), (1, 1)]),
        ("reversed within 64", 0, 0, [(s, 1) for s in range(60, 0, -1)]),
        ("jump of more than 64", 10, 0x3FF, [(200, 1), (199, 1), (136, 1), (137, 1), (10, 1)]),
        ("63 and 64 behind", 100, 1, [(37, 1), (36, 1)]),
        ("63 and 64 behind the batch's maximum", 0, 0, [(100, 1), (37, 1), (36, 1)]),
        ("twice and three times", 0, 0, [(5, 1), (5, 1), (7, 1), (7, 1), (7, 1), (6, 1)]),
        ("forged copy first", 0, 0, [(9, 0), (9, 1), (9, 1), (8, 0), (8, 1)]),
        ("bits of W0", 50, 0b1011, [(50, 1), (49, 1), (48, 1), (47, 1), (20, 1)]),
        ("older than the old window", 500, full, [(436, 1), (437, 1), (100, 1), (501, 1)]),
        ("full old window, then a shift", 500, full, [(437, 1), (600, 1), (537, 1), (536, 1)]),
        ("forged jump does not move the window", 10, 1, [(1000, 0), (11, 1), (9, 1)]),
    ]
