"""CPU: the plugin chain's surface that needs no GPU -- tests/chain_model.py against hand-written cases for every
row of the two tables of include/qgcm.h "plugin chain on routed batches", the NULL-context contract of the new
entry points, the binding, and route.Router with the node's plugins (main.go:41-51 order)."""
import ctypes as C
import os
import re

import numpy as np

import chain_model as M
from conftest import ROOT
from oracle import oracle as O
from oracle import snappy_oracle as SO
from quantum_amd import _lib, common, plugin, route
from route_model import NO_PEER

NEW = ("qgcm_peer_plugins_set", "qgcm_peer_plugins_get", "qgcm_chain_outgoing", "qgcm_chain_incoming",
       "qgcm_route_account_bytes", "qgcm_route_chain_seal_host", "qgcm_route_chain_open_host")
STRIDE = 64
BOTH = M.COMPRESSION | M.ENCRYPTION


def le(s: str) -> int:
    a, b, c, d = (int(x) for x in s.split("."))
    return a | b << 8 | c << 16 | d << 24


OWN = le("10.99.0.1")
# peers 0..3: flags 0..3, keyed; peer 4: both plugins, key slot unset; peer 5: never given flags (ENCRYPTION), keyed
NET = M.Net({le(f"10.99.0.{10 + p}"): p for p in range(6)}, le("10.99.0.0"), le("255.255.0.0"), le("10.99.7.7"), OWN)
KEYS = {p: bytes(range(p, p + 32)) for p in (0, 1, 2, 3, 5)}
PEERS = M.Peers({0: 0, 1: 1, 2: 2, 3: 3, 4: 3}, KEYS, 8)
NONCE = bytes(range(100, 112))


def tun_slot(peer, L, fill=None):
    """A TUN frame for `peer` (None: a stranger): distinct bytes, so snappy stores it as one literal."""
    s = np.zeros(STRIDE, np.uint8)
    s[0:4] = 0xEE
    s[4:4 + L] = np.arange(1, L + 1, dtype=np.uint8) * 7 if fill is None else fill
    dst = le("10.99.9.9") if peer is None else le(f"10.99.0.{10 + peer}")
    s[20:24] = np.frombuffer(dst.to_bytes(4, "little"), np.uint8)
    return s


def literal(pkt: bytes) -> bytes:
    """The snappy stream of a short incompressible packet, by hand: uvarint length, one literal element."""
    assert len(pkt) < 60
    return bytes([len(pkt), (len(pkt) - 1) << 2]) + pkt


def run_out(slot, L, plugins=BOTH, nonce=NONCE):
    return M.outgoing(NET, PEERS, slot[None, :].copy(), [L], plugins, None if nonce is None else np.frombuffer(nonce, np.uint8)[None, :])


def one(res):
    return int(res.lens[0]), int(res.status[0]), int(res.nbytes[0])


def test_outgoing_rows():
    own = np.frombuffer(OWN.to_bytes(4, "little"), np.uint8)
    # unresolved: slot untouched, nothing counted but a dropped packet in the totals
    s = tun_slot(None, 24)
    r = run_out(s, 24)
    assert one(r) == (0, 0, 0) and np.array_equal(r.slots[0], s) and r.peer[0] == NO_PEER
    assert r.totals.tolist() == [0, 0, 1, 0] and not r.links.any()
    # too short to hold a destination, or no room for tag and nonce: unresolved as well
    assert one(run_out(tun_slot(3, 19), 19)) == (0, 0, 0) and one(run_out(tun_slot(3, 33), 33)) == (0, 0, 0)
    # no plugin in F: passed through byte for byte (own_ip written by the resolve)
    for peer, plugins in ((0, BOTH), (3, 0), (1, M.ENCRYPTION), (2, M.COMPRESSION)):
        s = tun_slot(peer, 24)
        r = run_out(s, 24, plugins)
        want = s.copy()
        want[0:4] = own
        assert one(r) == (28, 1, 28) and np.array_equal(r.slots[0], want), peer
        assert r.links[peer].tolist() == [1, 28, 0, 0] and r.totals.tolist() == [1, 28, 0, 0]
    # compression only: Raw[4:] <- the stream, L <- its length
    s = tun_slot(1, 24)
    r = run_out(s, 24)
    stream = literal(bytes(s[4:28]))
    assert one(r) == (4 + 26, 1, 4 + 26) and bytes(r.slots[0][4:30]) == stream and bytes(r.slots[0][30:]) == bytes(s[30:])
    # encryption only: ct | tag | nonce under the peer's key, AAD Raw[0:4]
    s = tun_slot(2, 24)
    r = run_out(s, 24)
    ct, tag = O.gcm_seal(KEYS[2], NONCE, OWN.to_bytes(4, "little"), bytes(s[4:28]))
    assert one(r) == (56, 1, 56) and bytes(r.slots[0][:56]) == OWN.to_bytes(4, "little") + ct + tag + NONCE
    assert one(run_out(tun_slot(5, 24), 24)) == (56, 1, 56)  # a peer whose flags were never set: ENCRYPTION
    # both: the stream is what gets sealed
    s = tun_slot(3, 24)
    r = run_out(s, 24)
    ct, tag = O.gcm_seal(KEYS[3], NONCE, OWN.to_bytes(4, "little"), literal(bytes(s[4:28])))
    assert one(r) == (4 + 26 + 28, 1, 58) and bytes(r.slots[0][4:58]) == ct + tag + NONCE
    # ... with the nonce taken from the slot when no array is given
    s[4 + 26 + 16:4 + 26 + 28] = np.frombuffer(NONCE, np.uint8)
    assert np.array_equal(run_out(s, 24, nonce=None).slots[0][:58], r.slots[0][:58])
    # the codec refuses: 31 incompressible bytes make a 33-byte stream, 1 more than stride - 4 - 28 ...
    s = tun_slot(3, 31)
    r = run_out(s, 31)
    want = s.copy()
    want[0:4] = own
    assert one(r) == (0, 0, 35) and np.array_equal(r.slots[0], want) and r.links[3].tolist() == [0, 0, 1, 35]
    # ... but not more than stride - 4 for a peer that does not encrypt
    s = tun_slot(1, 31)
    assert one(run_out(s, 31)) == (4 + 33, 1, 4 + 33)
    # key slot unset: dropped with the (compressed) packet in the slot, Length at that point
    s = tun_slot(4, 24)
    r = run_out(s, 24)
    assert one(r) == (0, 0, 4 + 26) and bytes(r.slots[0][4:30]) == literal(bytes(s[4:28])) and r.links[4].tolist() == [0, 0, 1, 30]
    r = run_out(s, 24, M.ENCRYPTION)
    assert one(r) == (0, 0, 28) and bytes(r.slots[0][4:]) == bytes(s[4:])
    # a compressible packet shrinks, and decodes back
    s = tun_slot(1, 32, fill=0x41)
    r = run_out(s, 32)
    n = int(r.lens[0]) - 4
    assert n < 32 and SO.decode(bytes(r.slots[0][4:4 + n])) == bytes(s[4:36])


def datagram(sender, packet: bytes):
    s = np.full(STRIDE, 0xEE, np.uint8)
    s[0:4] = np.frombuffer((le("10.99.9.9") if sender is None else le(f"10.99.0.{10 + sender}")).to_bytes(4, "little"), np.uint8)
    s[4:4 + len(packet)] = np.frombuffer(packet, np.uint8)
    return s, 4 + len(packet)


def sealed(peer, pt: bytes) -> bytes:
    ct, tag = O.gcm_seal(KEYS[peer], NONCE, le(f"10.99.0.{10 + peer}").to_bytes(4, "little"), pt)
    return ct + tag + NONCE


def run_in(s, m, plugins=BOTH):
    return M.incoming(NET, PEERS, s[None, :].copy(), [m], plugins)


def test_incoming_rows():
    pkt = bytes(range(50, 70))
    # unresolved: an unknown sender, a datagram without a whole address, one longer than the slot
    for s, m in (datagram(None, pkt), (datagram(3, b"")[0], 3), (datagram(3, b"")[0], 0), (datagram(3, pkt)[0], STRIDE + 4)):
        r = run_in(s, m)
        assert one(r) == (0, 0, 0) and np.array_equal(r.slots[0], s) and r.totals.tolist() == [0, 0, 1, 0]
    # delivered, each combination (F = 0: untouched; also an empty packet: status 1 with length 0)
    s, m = datagram(0, pkt)
    r = run_in(s, m)
    assert one(r) == (20, 1, 24) and np.array_equal(r.slots[0], s)
    assert one(run_in(*datagram(0, b""))) == (0, 1, 4)
    s, m = datagram(1, literal(pkt))
    r = run_in(s, m)
    assert one(r) == (20, 1, 24) and bytes(r.slots[0][4:24]) == pkt and bytes(r.slots[0][24:]) == bytes(s[24:])
    s, m = datagram(2, sealed(2, pkt))
    r = run_in(s, m)
    assert m == 52 and one(r) == (20, 1, 24) and bytes(r.slots[0][4:24]) == pkt and not r.specified[0]
    s, m = datagram(3, sealed(3, literal(pkt)))
    r = run_in(s, m)
    assert m == 54 and one(r) == (20, 1, 24) and bytes(r.slots[0][4:24]) == pkt
    assert r.links[3].tolist() == [1, 24, 0, 0] and r.totals.tolist() == [1, 24, 0, 0]
    # the node's own mask gates too: without compression the opened stream is delivered as it is
    r = run_in(s, m, M.ENCRYPTION)
    assert one(r) == (22, 1, 26) and bytes(r.slots[0][4:26]) == literal(pkt)
    # the open fails: a flipped tag bit zeroes the plaintext region and leaves the rest; bytes = m
    s, m = datagram(3, sealed(3, literal(pkt)))
    s[4 + 22 + 3] ^= 0x10
    r = run_in(s, m)
    want = s.copy()
    want[4:26] = 0
    assert one(r) == (0, 0, 54) and np.array_equal(r.slots[0], want) and r.links[3].tolist() == [0, 0, 1, 54]
    # ... an unset key slot or a packet shorter than tag and nonce leave the slot alone
    for s, m in (datagram(4, sealed(3, pkt)), datagram(2, bytes(27)), datagram(2, b"")):
        r = run_in(s, m)
        assert one(r) == (0, 0, m) and np.array_equal(r.slots[0], s)
    # the decode fails: not a stream, an empty result, a header that claims more than the slot holds
    cut = bytes([61, 0x00, 0x41, 0xEE, 0x01])  # a literal, then a copy element cut short
    for bad in (bytes([200, 1, 2, 3, 4, 5]), b"\x00", cut, b""):
        s, m = datagram(1, bad)
        r = run_in(s, m)
        assert one(r) == (0, 0, 4 + len(bad)) and np.array_equal(r.slots[0], s), bad
        # ... after an open: DroppedBytes is the length after the open, the slot holds the opened packet
        s, m = datagram(3, sealed(3, bad))
        r = run_in(s, m)
        assert one(r) == (0, 0, 4 + len(bad)) and bytes(r.slots[0][4:4 + len(bad)]) == bad
    # a well-formed stream of 61 bytes in a 64-byte slot: one more than stride - 4
    rep = bytes([61, 0x00, 0x41, 0xEE, 0x01, 0x00])  # literal "A", copy of 60 bytes at offset 1
    assert SO.decode(rep) == b"A" * 61
    assert one(run_in(*datagram(1, rep))) == (0, 0, 4 + len(rep))
    rep60 = bytes([60, 0x00, 0x41, 0xEA, 0x01, 0x00])
    assert one(run_in(*datagram(1, rep60))) == (60, 1, 64)


def test_batch_counters_add_up():
    slots = np.stack([tun_slot(p, L) for p, L in ((None, 24), (3, 24), (3, 31), (1, 24), (4, 24), (0, 24), (3, 24))])
    r = M.outgoing(NET, PEERS, slots, [24, 24, 31, 24, 24, 24, 24], BOTH, np.tile(np.frombuffer(NONCE, np.uint8), (7, 1)))
    assert r.status.tolist() == [0, 1, 0, 1, 0, 1, 1] and r.nbytes.tolist() == [0, 58, 35, 30, 30, 28, 58]
    assert r.totals.tolist() == [4, 58 + 30 + 28 + 58, 3, 35 + 30]
    assert r.links[3].tolist() == [2, 116, 1, 35] and r.links[4].tolist() == [0, 0, 1, 30] and r.links[2].tolist() == [0] * 4
    assert r.links.sum(axis=0).tolist() == [4, 174, 2, 65]  # the unresolved packet is in the totals only


def test_header_declares_and_binding_holds_the_new_calls():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qgcm.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(qgcm_[a-z0-9_]+)\s*\(", text))
    L = _lib.lib()
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS and hasattr(L, name), name
    assert re.search(r"#define QGCM_PLUGIN_COMPRESSION 1u\b", text) and re.search(r"#define QGCM_PLUGIN_ENCRYPTION +2u\b", text)
    assert (_lib.PLUGIN_COMPRESSION, _lib.PLUGIN_ENCRYPTION) == (M.COMPRESSION, M.ENCRYPTION) == (1, 2)
    assert "#define QGCM_CHAIN_WORK(n)" in text
    for n in (0, 1, 16, 17, 65537):
        assert _lib.chain_work(n) % 16 == 0 and 4 * n <= _lib.chain_work(n) <= max(8 * n, 64)


def test_null_context_is_an_argument_error():
    L = _lib.lib()
    buf = (C.c_uint8 * 256)()
    p = C.addressof(buf)
    assert L.qgcm_peer_plugins_set(None, 0, 1, p) == _lib.QGCM_E_ARG
    assert L.qgcm_peer_plugins_get(None, 0, 1, p) == _lib.QGCM_E_ARG
    assert L.qgcm_chain_outgoing(None, p, 64, 1, p, p, p, 3, None, p, p, p, None) == _lib.QGCM_E_ARG
    assert L.qgcm_chain_incoming(None, p, 64, 1, p, p, p, 3, p, p, p, None) == _lib.QGCM_E_ARG
    assert L.qgcm_route_account_bytes(None, _lib.TX, 1, p, p, p, None) == _lib.QGCM_E_ARG
    assert L.qgcm_route_chain_seal_host(None, p, 64, 1, p, None, 3, p, None) == _lib.QGCM_E_ARG
    assert L.qgcm_route_chain_open_host(None, p, 64, 1, p, 3, p, None) == _lib.QGCM_E_ARG
    # n == 0 does not excuse the missing context either
    assert L.qgcm_chain_outgoing(None, None, 64, 0, None, None, None, 0, None, None, None, None, None) == _lib.QGCM_E_ARG
    assert L.qgcm_route_account_bytes(None, _lib.RX, 0, None, None, None, None) == _lib.QGCM_E_ARG


def test_peer_plugins_set_rejects_without_a_gpu():
    """No context can exist without a GPU, so every call is refused for that already; flag 4 and a range past
    max_keys are QGCM_E_ARG whichever check sees them first (the GPU suite repeats both on a live context)."""
    L = _lib.lib()
    assert L.qgcm_peer_plugins_set(None, 0, 1, bytes([4])) == _lib.QGCM_E_ARG
    assert L.qgcm_peer_plugins_set(None, 0xFFFFFFFF, 2, bytes([2, 2])) == _lib.QGCM_E_ARG
    assert L.qgcm_peer_plugins_get(None, 0xFFFFFFFF, 2, C.addressof((C.c_uint8 * 2)())) == _lib.QGCM_E_ARG


def test_plugin_flags():
    assert route.plugin_flags(None) == 0 and route.plugin_flags(["mock"]) == 0
    assert route.plugin_flags(["compression"]) == 1 and route.plugin_flags(["encryption", "mock"]) == 2
    assert route.plugin_flags(["encryption", "compression"]) == 3


class Xor:
    """A stand-in for crypto.AES (which needs a GPU): Encrypt / Decrypt with crypto/aes.go's sizes."""

    def Encrypt(self, data, length, aad):  # data: a common._View of Raw[4:]
        buf, o = data.buf, data.start
        for i in range(length):
            buf[o + i] ^= 0x5A
        buf[o + length:o + length + 28] = bytes(0xA0 + i for i in range(28))
        return length + 28, None

    def Decrypt(self, data, aad):
        buf, o, n = data.buf, data.start, len(data) - 28
        if n < 0 or bytes(buf[o + n:o + n + 28]) != bytes(0xA0 + i for i in range(28)):
            return 0, ValueError("open")
        for i in range(n):
            buf[o + i] ^= 0x5A
        return n, None


def test_router_applies_the_plugins_in_the_reference_order():
    pkt = bytes(20) + b"quantum " * 10
    maps = {le(f"10.99.0.{10 + k}"): common.Mapping(SupportedPlugins=names, AES=Xor())
            for k, names in enumerate(([], ["compression"], ["encryption"], ["compression", "encryption"]))}
    # given in the wrong order on purpose: main.go:46-51 sorts them
    r = route.Router(maps, le("10.99.0.0"), le("255.255.0.0"), le("10.99.7.7"), OWN, plugins=["encryption", "compression"])
    assert [p.Name() for p in r.plugins[0]] == ["compression", "encryption"]
    assert [p.Name() for p in r.plugins[1]] == ["encryption", "compression"]
    stream = SO.encode(pkt[:16] + bytes([10, 99, 0, 13]) + pkt[20:])
    for k in range(4):
        raw = bytearray(256)
        body = pkt[:16] + bytes([10, 99, 0, 10 + k]) + pkt[20:]
        raw[4:4 + len(body)] = body
        pl, mapping, ok = r.outgoing(common.NewTunPayload(raw, len(body)))
        assert ok and mapping is maps[le(f"10.99.0.{10 + k}")] and bytes(raw[0:4]) == OWN.to_bytes(4, "little")
        want = SO.encode(body) if k & 1 else body
        if k & 2:
            want = bytes(b ^ 0x5A for b in want) + bytes(0xA0 + i for i in range(28))
        assert pl.Length == 4 + len(want) and bytes(raw[4:4 + len(want)]) == want, k
        # the same datagram back in, from that peer: encryption first, then compression
        raw[0:4] = bytes([10, 99, 0, 10 + k])
        pl, mapping, ok = r.incoming(common.NewSockPayload(raw, pl.Length))
        assert ok and pl.Length == 4 + len(body) and bytes(raw[4:4 + len(body)]) == body, k
    assert len(stream) < len(pkt)
    # a plugin that drops the packet ends the chain: not a stream, for the compressing peer
    raw = bytearray(bytes([10, 99, 0, 11]) + b"\xc8\x01\x02\x03" + bytes(56))
    pl, mapping, ok = r.incoming(common.NewSockPayload(raw, 8))
    assert not ok and pl.Length == 8
    # without plugins the router only resolves, as before
    plain = route.Router(maps, le("10.99.0.0"), le("255.255.0.0"), le("10.99.7.7"), OWN)
    raw = bytearray(64)
    raw[20:24] = bytes([10, 99, 0, 13])
    pl, mapping, ok = plain.outgoing(common.NewTunPayload(raw, 40))
    assert ok and pl.Length == 44 and bytes(raw[4:20]) == bytes(16)
    assert isinstance(plugin.New("compression")[0], plugin.Compression)
