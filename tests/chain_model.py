"""A per-packet CPU model of the plugin chain on routed batches (include/qgcm.h "plugin chain on routed
batches"), shared by tests/test_chain_model.py and tests/test_gpu_chain_route.py.

The two tables of the header, written out one packet at a time: resolve over a plain dict (router/router.go:21-31
with the batch calls' documented misses), then F = plugins & flags[peer], compression before encryption outgoing
and the reverse incoming, and the payload.Length that worker/outgoing.go:37-53 counts.  GCM is oracle/oracle.py,
snappy is oracle/snappy_oracle.py: neither shares code with the library.  Counters are summed here, packet by
packet, in the layout tests/route_model.py uses: totals of shape (4,), links of shape (max_keys, 4), columns
[Packets, Bytes, DroppedPackets, DroppedBytes].
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from oracle import oracle as O
from oracle import snappy_oracle as SO
from route_model import NO_PEER, OVERHEAD

COMPRESSION, ENCRYPTION = 1, 2
SNAPPY_DEVICE_MAX = 16384


@dataclass
class Net:
    """What a node resolves with: `table` maps IPtoInt address -> key slot."""

    table: dict
    net: int
    mask: int
    gateway: int
    own_ip: int

    def lookup(self, addr: int) -> int:
        key = addr if (addr & self.mask) == (self.net & self.mask) else self.gateway
        return self.table.get(key, NO_PEER)


@dataclass
class Peers:
    """`flags[p]` the peer's plugin byte (absent: ENCRYPTION, a slot's initial value), `keys[p]` its 32-byte
    key (absent: the slot is unset)."""

    flags: dict
    keys: dict
    max_keys: int

    def effective(self, plugins: int, peer: int) -> int:
        return plugins & self.flags.get(peer, ENCRYPTION)


@dataclass
class Result:
    slots: np.ndarray   # (n, stride) uint8
    lens: np.ndarray    # uint32
    status: np.ndarray  # uint8
    nbytes: np.ndarray  # uint32
    peer: np.ndarray    # uint32
    totals: np.ndarray  # (4,) uint64
    links: np.ndarray   # (max_keys, 4) uint64
    specified: np.ndarray  # bool: the whole slot is specified (else only Raw[:Length] of a delivered packet)


def resolve_out(net: Net, slot, L: int, stride: int, max_keys: int) -> int:
    """qgcm_resolve_outgoing for one slot: the peer, own_ip written on a hit."""
    if L < 20 or 4 + L + OVERHEAD > stride:
        return NO_PEER
    peer = net.lookup(int.from_bytes(bytes(slot[20:24]), "little"))
    if peer == NO_PEER:
        return NO_PEER
    slot[0:4] = np.frombuffer(net.own_ip.to_bytes(4, "little"), np.uint8)
    return peer if peer < max_keys else NO_PEER


def resolve_in(net: Net, slot, m: int, stride: int, max_keys: int) -> int:
    if m < 4 or m > stride:
        return NO_PEER
    peer = net.lookup(int.from_bytes(bytes(slot[0:4]), "little"))
    return peer if peer < max_keys else NO_PEER


def out_packet(slot, L: int, peer: int, F: int, key, nonce, stride: int):
    """One resolved outgoing packet, `slot` (uint8 array of `stride` bytes) changed in place ->
    (d_lens, status, bytes).  `nonce` None: the nonce is in the slot already."""
    if F & COMPRESSION:
        out = SO.encode(bytes(slot[4:4 + L])) if L <= SNAPPY_DEVICE_MAX else None
        if out is None or len(out) > stride - 4 - (OVERHEAD if F & ENCRYPTION else 0):
            return 0, 0, 4 + L  # refused: the slot as resolve left it
        slot[4:4 + len(out)] = np.frombuffer(out, np.uint8)
        L = len(out)
    if not F & ENCRYPTION:
        return 4 + L, 1, 4 + L
    if key is None:
        return 0, 0, 4 + L
    if nonce is None:
        nonce = bytes(slot[4 + L + 16:4 + L + OVERHEAD])
    buf = bytearray(bytes(slot[4:4 + L + OVERHEAD]))
    assert O.aesgo_encrypt(key, buf, L, bytes(slot[0:4]), bytes(nonce)) == L + OVERHEAD
    slot[4:4 + L + OVERHEAD] = np.frombuffer(bytes(buf), np.uint8)
    return 4 + L + OVERHEAD, 1, 4 + L + OVERHEAD


def in_packet(slot, m: int, peer: int, F: int, key, stride: int):
    """One resolved incoming datagram Raw[:m] -> (d_lens, status, bytes, whole slot specified)."""
    L = m - 4
    if F & ENCRYPTION:
        if L < OVERHEAD or key is None:
            return 0, 0, m, True  # slot untouched
        buf = bytearray(bytes(slot[4:4 + L]))
        if O.aesgo_decrypt(key, buf, bytes(slot[0:4])) != L - OVERHEAD:
            slot[4:4 + L - OVERHEAD] = 0  # tag mismatch: the plaintext region zeroed, as Go 1.9 gcm.Open does
            return 0, 0, m, True
        L -= OVERHEAD
        slot[4:4 + L] = np.frombuffer(bytes(buf[:L]), np.uint8)
    if F & COMPRESSION:
        out = SO.decode(bytes(slot[4:4 + L]))
        if out is None or len(out) == 0 or len(out) > min(stride - 4, SNAPPY_DEVICE_MAX):
            return 0, 0, 4 + L, True  # the slot keeps the packet the codec was given
        slot[4:4 + len(out)] = np.frombuffer(out, np.uint8)
        L = len(out)
    # an opened slot is specified up to its plaintext (qgcm_open_batch says nothing of the bytes behind it)
    return L, 1, 4 + L, not F & ENCRYPTION


def _count(totals, links, peer: int, status: int, nbytes: int) -> None:
    if peer == NO_PEER:
        totals[2] += np.uint64(1)
        return
    col = 0 if status == 1 else 2
    for row in (totals, links[peer]):
        row[col] += np.uint64(1)
        row[col + 1] += np.uint64(nbytes)


def outgoing(net: Net, peers: Peers, slots: np.ndarray, lens, plugins: int, nonces=None) -> Result:
    """qgcm_resolve_outgoing -> qgcm_chain_outgoing -> qgcm_route_account_bytes(TX) of a batch.  `nonces`:
    (n, 12) uint8, or None (each nonce is in its slot)."""
    n, stride = slots.shape
    res = _blank(slots, peers.max_keys)
    for i in range(n):
        slot, L = res.slots[i], int(lens[i])
        peer = resolve_out(net, slot, L, stride, peers.max_keys)
        res.peer[i] = peer
        if peer != NO_PEER:
            F = peers.effective(plugins, peer)
            nonce = None if nonces is None else bytes(nonces[i])
            res.lens[i], res.status[i], res.nbytes[i] = out_packet(slot, L, peer, F, peers.keys.get(peer), nonce, stride)
        _count(res.totals, res.links, peer, int(res.status[i]), int(res.nbytes[i]))
    return res


def incoming(net: Net, peers: Peers, slots: np.ndarray, lens, plugins: int) -> Result:
    """qgcm_resolve_incoming -> qgcm_chain_incoming -> qgcm_route_account_bytes(RX) of a batch."""
    n, stride = slots.shape
    res = _blank(slots, peers.max_keys)
    for i in range(n):
        slot, m = res.slots[i], int(lens[i])
        peer = resolve_in(net, slot, m, stride, peers.max_keys)
        res.peer[i] = peer
        if peer != NO_PEER:
            F = peers.effective(plugins, peer)
            res.lens[i], res.status[i], res.nbytes[i], res.specified[i] = in_packet(slot, m, peer, F, peers.keys.get(peer), stride)
        _count(res.totals, res.links, peer, int(res.status[i]), int(res.nbytes[i]))
    return res


def _blank(slots: np.ndarray, max_keys: int) -> Result:
    n = len(slots)
    return Result(slots.copy(), np.zeros(n, np.uint32), np.zeros(n, np.uint8), np.zeros(n, np.uint32),
                  np.full(n, NO_PEER, np.uint32), np.zeros(4, np.uint64), np.zeros((max_keys, 4), np.uint64),
                  np.ones(n, bool))
