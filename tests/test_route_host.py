"""CPU: the route surface of include/qgcm.h that needs no GPU -- the eight declarations and their binding,
the NULL-context contract, route.Router against router/router.go:21-31 restated here over a plain dict,
and qgcm_udp_send_slots_to (socket/udp.go:44-47 with mapping.Sockaddr per packet) over loopback."""
import ctypes as C
import os
import random
import re
import socket

import numpy as np

from conftest import ROOT
from quantum_amd import _lib, common, route

NEW = ("qgcm_routes_set", "qgcm_resolve_outgoing", "qgcm_resolve_incoming", "qgcm_route_account", "qgcm_route_stats",
       "qgcm_route_seal_host", "qgcm_route_open_host", "qgcm_udp_send_slots_to")
STRIDE = common.MaxPacketLength


def test_header_declares_and_binding_holds_the_new_calls():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qgcm.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(qgcm_[a-z0-9_]+)\s*\(", text))
    L = _lib.lib()
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS and hasattr(L, name), name
    assert "#define QGCM_NO_PEER 0xffffffffu" in text and _lib.NO_PEER == 0xFFFFFFFF
    assert re.search(r"#define QGCM_TX 0\b", text) and re.search(r"#define QGCM_RX 1\b", text)
    assert C.sizeof(_lib.Route) == 8 and C.sizeof(_lib.RouteNet) == 16 and C.sizeof(_lib.PeerAddr) == 8


def test_null_context_is_an_argument_error():
    L = _lib.lib()
    rn = _lib.RouteNet(0, 0, 0, 0)
    out = (C.c_uint64 * 4)()
    buf = (C.c_uint8 * 64)()
    p = C.addressof(buf)
    assert L.qgcm_routes_set(None, None, 0, C.addressof(rn)) == _lib.QGCM_E_ARG
    assert L.qgcm_resolve_outgoing(None, p, 64, 1, p, p, p, None) == _lib.QGCM_E_ARG
    assert L.qgcm_resolve_incoming(None, p, 64, 1, p, p, p, None) == _lib.QGCM_E_ARG
    assert L.qgcm_route_account(None, _lib.TX, 1, p, p, None, None) == _lib.QGCM_E_ARG
    assert L.qgcm_route_stats(None, _lib.TX, _lib.NO_PEER, C.addressof(out)) == _lib.QGCM_E_ARG
    assert L.qgcm_route_seal_host(None, p, 64, 1, p, None, p, None) == _lib.QGCM_E_ARG
    assert L.qgcm_route_open_host(None, p, 64, 1, p, p, None) == _lib.QGCM_E_ARG
    # n == 0 does not excuse the missing context either
    assert L.qgcm_resolve_outgoing(None, None, 64, 0, None, None, None, None) == _lib.QGCM_E_ARG


def ip(s: str) -> bytes:
    return socket.inet_aton(s)


def le(s: str) -> int:
    """common.IPtoInt written out: the first address byte is the least significant."""
    a, b, c, d = (int(x) for x in s.split("."))
    return a | b << 8 | c << 16 | d << 24


def expect(table: dict, net: int, mask: int, gateway: int, dst: int):
    """router.go:21-31 over a dict."""
    key = dst if (dst & mask) == (net & mask) else gateway
    return (table[key], True) if key in table else (None, False)


def test_iptoint_byte_order():
    assert route.IPtoInt(ip("10.99.0.1")) == 0x0100630A == le("10.99.0.1")
    assert route.IPtoInt(bytes([1, 0, 0, 0])) == 1 and route.IPtoInt(bytes([0, 0, 0, 1])) == 1 << 24
    assert route.mask_of(0) == 0 and route.mask_of(32) == 0xFFFFFFFF
    assert route.mask_of(16) == le("255.255.0.0") and route.mask_of(24) == le("255.255.255.0")


def test_router_resolve_cases():
    table = {le("10.99.0.1"): "a", le("10.99.0.2"): "b", le("10.99.7.1"): "gw",
             le("11.99.0.1"): "first-byte", le("10.99.0.3"): "c", le("0.0.0.0"): "zero"}
    net, mask = le("10.99.0.0"), le("255.255.0.0")
    r = route.Router(table, net, mask, le("10.99.7.1"), le("10.99.0.9"))
    assert r.Resolve(ip("10.99.0.1")) == ("a", True)               # a hit inside the net
    assert r.Resolve(ip("10.99.200.200")) == (None, False)         # a miss inside the net
    assert r.Resolve(ip("8.8.8.8")) == ("gw", True)                # outside: the mapped gateway
    assert r.Resolve(ip("11.99.0.1")) == ("gw", True)              # differs from a hit in its first byte only: outside
    assert r.Resolve(ip("10.99.0.2")) == ("b", True) and r.Resolve(ip("10.99.0.3")) == ("c", True)  # last byte only
    unmapped = route.Router(table, net, mask, le("10.99.7.2"), le("10.99.0.9"))
    assert unmapped.Resolve(ip("8.8.8.8")) == (None, False)        # outside: the gateway is not mapped
    everything = route.Router(table, le("0.0.0.0"), route.mask_of(0), le("10.99.7.1"), 0)
    assert everything.Resolve(ip("11.99.0.1")) == ("first-byte", True)   # /0: every address is inside
    assert everything.Resolve(ip("0.0.0.0")) == ("zero", True)           # 0.0.0.0 as a mapped key
    assert everything.Resolve(ip("9.9.9.9")) == (None, False)
    single = route.Router(table, le("10.99.0.1"), route.mask_of(32), le("10.99.0.2"), 0)
    assert single.Resolve(ip("10.99.0.1")) == ("a", True)          # /32: the one address inside
    assert single.Resolve(ip("10.99.0.3")) == ("b", True)          # its neighbour goes to the gateway
    rng = random.Random(0x2077)
    for _ in range(2000):
        dst = bytes(rng.choice([10, 11, 0]) if k == 0 else rng.choice([99, 0, 7]) if k == 1 else rng.randrange(4)
                    for k in range(4))
        for rt in (r, unmapped, everything, single):
            assert rt.Resolve(dst) == expect(table, rt.net, rt.mask, rt.gateway, int.from_bytes(dst, "little"))


def test_router_serves_the_per_packet_workers():
    """Router.outgoing / incoming are worker/outgoing.go:28-35 and incoming.go:28-34: the `resolve` of worker.py."""
    r = route.Router({le("10.99.0.2"): "peer"}, le("10.99.0.0"), le("255.255.0.0"), le("10.99.7.1"), le("10.99.0.1"))
    raw = bytearray(64)
    raw[4 + 16:4 + 20] = ip("10.99.0.2")
    pl, mapping, ok = r.outgoing(common.NewTunPayload(raw, 40))
    assert ok and mapping == "peer" and bytes(pl.Raw[0:4]) == ip("10.99.0.1")  # outgoing.go:30
    raw2 = bytearray(64)
    raw2[4 + 16:4 + 20] = ip("10.99.0.3")
    assert r.outgoing(common.NewTunPayload(raw2, 40)) == (None, None, False) and raw2[0:4] == bytes(4)
    raw3 = bytearray(ip("10.99.0.2") + bytes(60))
    assert r.incoming(common.NewSockPayload(raw3, 64))[1:] == ("peer", True)
    raw3[0:4] = ip("10.99.0.4")
    assert r.incoming(common.NewSockPayload(raw3, 64)) == (None, None, False)


def test_udp_send_slots_to_delivers_each_packet_to_its_peer():
    L = _lib.lib()
    tx = L.qgcm_udp_socket(b"127.0.0.1", 0, 1 << 22)
    rx = [L.qgcm_udp_socket(b"127.0.0.1", 0, 1 << 22) for _ in range(3)]
    assert tx >= 0 and all(f >= 0 for f in rx)
    try:
        rng = random.Random(0x70AD)
        n = 64
        peer = np.array([i % 3 for i in range(n)], np.uint32)
        lens = np.array([rng.choice([4, 33, 1382, STRIDE]) if i % 5 == 0 else rng.randint(4, STRIDE) for i in range(n)],
                        np.uint32)
        for i in (7, 20, 41):
            peer[i] = _lib.NO_PEER
        for i in (3, 30, 58):
            lens[i] = 0
        arena = np.frombuffer(rng.randbytes(n * STRIDE), np.uint8).copy()
        addrs = route.peer_addrs([("127.0.0.1", L.qgcm_udp_port(f)) for f in rx])
        want = [[i for i in range(n) if peer[i] == k and lens[i]] for k in range(3)]
        sent = route.udp_send_slots_to(tx, arena.ctypes.data, STRIDE, n, lens, peer, addrs, 3)
        assert sent == sum(len(w) for w in want) == n - 6
        for k, fd in enumerate(rx):
            got = np.zeros((len(want[k]) + 4) * STRIDE, np.uint8)
            got_lens = np.zeros(len(want[k]) + 4, np.uint32)
            m = 0
            while m < len(want[k]):
                r = L.qgcm_udp_recv_slots(fd, got[m * STRIDE:].ctypes.data, STRIDE, len(got_lens) - m,
                                          got_lens[m:].ctypes.data, 2000)
                assert r > 0, f"peer {k}: {m} of {len(want[k])} datagrams arrived"
                m += r
            assert m == len(want[k])  # exactly its own ...
            for j, i in enumerate(want[k]):  # ... in order, byte for byte
                assert got_lens[j] == lens[i], (k, i)
                assert np.array_equal(got[j * STRIDE:j * STRIDE + int(lens[i])], arena[i * STRIDE:i * STRIDE + int(lens[i])])
            # ... and nothing else
            assert L.qgcm_udp_recv_slots(fd, got.ctypes.data, STRIDE, 4, got_lens.ctypes.data, 0) == 0
        # a peer past the address table fails the call before anything is sent
        peer[10] = 3
        assert route.udp_send_slots_to(tx, arena.ctypes.data, STRIDE, n, lens, peer, addrs, 3) == -1
        for fd in rx:
            assert L.qgcm_udp_recv_slots(fd, got.ctypes.data, STRIDE, 4, got_lens.ctypes.data, 0) == 0
        # ... unless the packet is skipped anyway
        lens[10] = 0
        assert route.udp_send_slots_to(tx, arena.ctypes.data, STRIDE, 4, lens, peer, addrs, 3) == 3  # slot 3 has length 0
    finally:
        for f in [tx] + rx:
            L.qgcm_udp_close(f)
