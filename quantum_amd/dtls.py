"""DTLS 1.2 records on routed batches (include/qgcm.h "DTLS 1.2 records on routed batches"): the record layer
of quantum's `dtls` backend (socket/dtls.go, crypto/dtls.c) for established sessions, as GPU batches.

Sessions are indexed like peers; a session owns two key slots of the context.  The slot holds ciphertext | tag
at Raw[0 : L + 16]; the record header and explicit nonce (21 bytes) live in a side array of 32-byte entries.
Device arrays are torch tensors (uint8 arena / hdr / status / reason, int32 lens / peer)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from .route import _ptr, _stream_handle

OK, NO_SESSION, NOT_APPDATA, MALFORMED, AUTH, REPLAY, SEQ_EXHAUSTED = range(7)  # QGCM_DTLS_*
MAX_PLAIN = 16384  # QGCM_DTLS_MAX_PLAIN
HDR_BYTES = 21     # QGCM_DTLS_HDR_BYTES: record header and explicit nonce
HDR_ENTRY = 32     # sizeof(qgcm_dtls_hdr)
SEQ_END = 1 << 48


@dataclass
class Session:
    """One direction pair of an established session: what qgcm_dtls_keys carries."""

    write_key: bytes
    read_key: bytes
    write_iv: bytes
    read_iv: bytes
    write_slot: int
    read_slot: int
    write_epoch: int = 1
    read_epoch: int = 1
    write_seq: int = 0

    def mirrored(self, write_slot: int, read_slot: int, write_seq: int = 0) -> "Session":
        """The peer's view: its read side is this write side."""
        return Session(self.read_key, self.write_key, self.read_iv, self.write_iv, write_slot, read_slot,
                       self.read_epoch, self.write_epoch, write_seq)


def keys_array(sessions) -> C.Array:
    arr = (_lib.DtlsKeys * max(1, len(sessions)))()
    for a, s in zip(arr, sessions):
        assert len(s.write_key) == 32 and len(s.read_key) == 32 and len(s.write_iv) == 4 and len(s.read_iv) == 4
        a.write_key[:] = s.write_key
        a.read_key[:] = s.read_key
        a.write_iv[:] = s.write_iv
        a.read_iv[:] = s.read_iv
        a.write_epoch, a.read_epoch = s.write_epoch, s.read_epoch
        a.write_slot, a.read_slot = s.write_slot, s.read_slot
        a.write_seq = s.write_seq
    return arr


def sessions_set(ctx, first: int, sessions) -> None:
    arr = keys_array(sessions)
    _lib.check(_lib.lib().qgcm_dtls_sessions_set(ctx.handle, first, len(sessions), C.addressof(arr)),
               "qgcm_dtls_sessions_set")


def sessions_clear(ctx, first: int, count: int) -> None:
    _lib.check(_lib.lib().qgcm_dtls_sessions_clear(ctx.handle, first, count), "qgcm_dtls_sessions_clear")


def session_state(ctx, session: int) -> dict[str, int]:
    out = (C.c_uint64 * 4)()
    _lib.check(_lib.lib().qgcm_dtls_session_state(ctx.handle, session, C.addressof(out)), "qgcm_dtls_session_state")
    return {"write_seq": out[0], "R": out[1], "W": out[2], "set": out[3]}


def key_block(master: bytes, client_random: bytes, server_random: bytes) -> bytes:
    """PRF_SHA384(master, "key expansion", server_random | client_random), 72 bytes, on the host."""
    assert len(master) == 48 and len(client_random) == 32 and len(server_random) == 32
    out = C.create_string_buffer(72)
    _lib.check(_lib.lib().qgcm_dtls_key_block(master, client_random, server_random, out), "qgcm_dtls_key_block")
    return out.raw


def seal(ctx, arena, stride: int, n: int, lens, peer, hdr, status, reason=None, stream=None) -> None:
    _lib.check(_lib.lib().qgcm_dtls_seal(ctx.handle, _ptr(arena), stride, n, _ptr(lens), _ptr(peer), _ptr(hdr),
                                         _ptr(status), _ptr(reason), _stream_handle(stream)), "qgcm_dtls_seal")


def open(ctx, arena, stride: int, n: int, lens, peer, hdr, status, reason=None, stream=None) -> None:  # noqa: A001
    _lib.check(_lib.lib().qgcm_dtls_open(ctx.handle, _ptr(arena), stride, n, _ptr(lens), _ptr(peer), _ptr(hdr),
                                         _ptr(status), _ptr(reason), _stream_handle(stream)), "qgcm_dtls_open")


def number_cpu(sessions, is_set, write_seq, stride: int, lens, peer):
    """qgcm_dtls_number_cpu over numpy arrays: returns (hdr [n, 32] uint8, status, reason); lens (uint32) and
    write_seq (uint64) are updated in place."""
    n = len(lens)
    arr = keys_array(sessions)
    peer = np.ascontiguousarray(peer, np.uint32)
    hdr = np.full((max(1, n), HDR_ENTRY), 0xEE, np.uint8)
    status, reason = np.full(max(1, n), 0xEE, np.uint8), np.full(max(1, n), 0xEE, np.uint8)
    st = None if is_set is None else np.ascontiguousarray(is_set, np.uint8)
    _lib.check(_lib.lib().qgcm_dtls_number_cpu(C.addressof(arr), None if st is None else st.ctypes.data,
                                               write_seq.ctypes.data, len(sessions), stride, n, lens.ctypes.data,
                                               peer.ctypes.data, hdr.ctypes.data, status.ctypes.data,
                                               reason.ctypes.data), "qgcm_dtls_number_cpu")
    return hdr[:n], status[:n], reason[:n]


def replay_cpu(session, seq, authentic, state, parallel: bool = True):
    """qgcm_dtls_replay_cpu: accept flags (uint8) of n packets; state (uint64 [n_sessions, 2] = R, W) in place."""
    session = np.ascontiguousarray(session, np.uint32)
    seq = np.ascontiguousarray(seq, np.uint64)
    authentic = np.ascontiguousarray(authentic, np.uint8)
    n = len(session)
    accept = np.full(max(1, n), 0xEE, np.uint8)
    assert state.dtype == np.uint64 and state.flags.c_contiguous
    _lib.check(_lib.lib().qgcm_dtls_replay_cpu(n, session.ctypes.data, seq.ctypes.data, authentic.ctypes.data,
                                               state.shape[0], state.ctypes.data, accept.ctypes.data,
                                               1 if parallel else 0), "qgcm_dtls_replay_cpu")
    return accept[:n]


def udp_send_dtls(fd: int, arena_ptr: int, stride: int, n: int, lens, hdr, status, peer, addrs: C.Array,
                  n_addrs: int) -> int:
    """Datagram i = hdr[i][:21] | Raw[:lens[i]] to addrs[peer[i]] for the slots with status 1 (None: all)."""
    return _lib.lib().qgcm_udp_send_dtls(fd, arena_ptr, stride, n, lens.ctypes.data, hdr.ctypes.data,
                                         None if status is None else status.ctypes.data, peer.ctypes.data,
                                         C.addressof(addrs), n_addrs)


def udp_recv_dtls(fd: int, arena_ptr: int, stride: int, max_n: int, lens, hdr, addrs_out=None,
                  timeout_ms: int = 0) -> tuple[int, int]:
    """-> (slots filled, datagrams dropped)."""
    dropped = C.c_uint32(0)
    got = _lib.lib().qgcm_udp_recv_dtls(fd, arena_ptr, stride, max_n, lens.ctypes.data, hdr.ctypes.data,
                                        None if addrs_out is None else C.addressof(addrs_out), timeout_ms,
                                        C.addressof(dropped))
    return got, dropped.value
