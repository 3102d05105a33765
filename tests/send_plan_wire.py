"""Loopback plumbing shared by the send-plan tests: receiver sockets, draining, the UDP_SEGMENT probe."""
import socket
import struct

import numpy as np

from quantum_amd import _lib, route

STRIDE = 1472
UDP_SEGMENT = 103  # linux/udp.h


class Wire:
    """One sender and `peers` receivers on 127.0.0.1 (4 MiB socket buffers, as tests/test_udp_batch.py); peer p's
    address is addrs[p]."""

    def __init__(self, peers: int):
        self.L = _lib.lib()
        self.tx = self.L.qgcm_udp_socket(b"127.0.0.1", 0, 1 << 22)
        self.rx = [self.L.qgcm_udp_socket(b"127.0.0.1", 0, 1 << 22) for _ in range(peers)]
        assert self.tx >= 0 and all(fd >= 0 for fd in self.rx)
        self.addrs = route.peer_addrs([("127.0.0.1", self.L.qgcm_udp_port(fd)) for fd in self.rx])
        self.n_addrs = peers

    def close(self):
        for fd in [self.tx] + self.rx:
            self.L.qgcm_udp_close(fd)

    def send(self, slots, lens, order, trains, stats=None, n_addrs=None):
        """qgcm_udp_send_plan over `slots` (n, stride) uint8."""
        n, stride = slots.shape
        return route.udp_send_plan(self.tx, slots.ctypes.data, stride, n, np.ascontiguousarray(lens, np.uint32),
                                   np.ascontiguousarray(order, np.uint32),
                                   np.ascontiguousarray(trains, np.uint32).reshape(-1, 4), self.addrs,
                                   self.n_addrs if n_addrs is None else n_addrs, stats)

    def drain(self, p: int, want: int, timeout_ms: int = 1000):
        """The datagrams queued for peer p, in arrival order, until `want` have come or nothing comes."""
        cap = max(want, 1) + 8
        buf, ln, got = np.zeros((cap, STRIDE), np.uint8), np.zeros(cap, np.uint32), 0
        while got < want + 8:
            r = self.L.qgcm_udp_recv_slots(self.rx[p], buf[got:].ctypes.data, STRIDE, cap - got, ln[got:].ctypes.data,
                                           timeout_ms if got < want else 10)
            assert r >= 0
            if r == 0:
                break
            got += r
        return [buf[i, :ln[i]].tobytes() for i in range(got)]

    def nothing_arrived(self):
        buf, ln = np.zeros((4, STRIDE), np.uint8), np.zeros(4, np.uint32)
        return all(self.L.qgcm_udp_recv_slots(fd, buf.ctypes.data, STRIDE, 4, ln.ctypes.data, 10) == 0 for fd in self.rx)


def expected(slots, lens, peer, p):
    """Peer p's datagrams in arena order: what qgcm_udp_send_slots_to would send there."""
    return [slots[i, :lens[i]].tobytes() for i in range(len(lens)) if peer[i] == p and lens[i] != 0]


def gso_probe() -> bool:
    """Whether this kernel's loopback takes a UDP_SEGMENT message: two 10-byte segments from a plain socket."""
    rx = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
    tx = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
    try:
        rx.bind(("127.0.0.1", 0))
        rx.settimeout(1.0)
        tx.sendmsg([b"a" * 10, b"b" * 10], [(socket.IPPROTO_UDP, UDP_SEGMENT, struct.pack("H", 10))], 0, rx.getsockname())
        return [rx.recv(100), rx.recv(100)] == [b"a" * 10, b"b" * 10]
    except OSError:
        return False
    finally:
        rx.close()
        tx.close()
