"""CPU: qgcm_tun_open_offload and qgcm_tun_read_gso on a real TUN queue with IFF_VNET_HDR: what the kernel hands over
for a UDP_SEGMENT message and for a TCP sendall -- super-frames, or packets whose checksum it left to the reader --
read into a packed area and a table, cut by qgcm_gso_unpack_cpu, and checked as packets with a plain RFC 1071
routine.  Needs /dev/net/tun and CAP_NET_ADMIN; skipped where the device or TUNSETOFFLOAD is refused."""
import os
import socket
import struct
from ctypes import c_int as C_int

import numpy as np
import pytest

import gso_model as M
from quantum_amd import _lib, route

HOST_IP, PEER_IP = "10.213.9.1", "10.213.9.2"
STRIDE = 1536
UDP_SEGMENT = 103  # linux/udp.h


def open_tun(offloads):
    rc, fds, name = route.tun_open_offload(b"qgcmg%d", 1, offloads)
    if rc < 0:
        pytest.skip(f"offload TUN refused (errno {-rc})")
    if _lib.lib().qgcm_tun_up(name, HOST_IP.encode(), 24, 1433) < 0:
        _lib.lib().qgcm_tun_close(fds[0])
        pytest.skip("TUN link set-up refused")
    return fds[0]


@pytest.fixture()
def tun():
    fd = open_tun(_lib.TUN_TSO4)
    yield fd
    _lib.lib().qgcm_tun_close(fd)


class Reader:
    """qgcm_tun_read_gso then qgcm_gso_unpack_cpu, call after call: the IPv4 packets of `proto` to PEER_IP."""

    def __init__(self, fd, proto):
        self.fd, self.proto = fd, proto
        self.packed, self.frames = np.zeros(1 << 20, np.uint8), np.zeros(64, M.FRAME)
        self.kinds, self.packets, self.unsplit = [], [], 0

    def read(self, timeout_ms=50):
        out = np.zeros(3, np.uint64)
        n = route.tun_read_gso(self.fd, self.packed, self.frames, 8192, timeout_ms, out)
        assert n >= 0
        if n == 0:
            return 0
        table = self.frames[:int(out[0])]
        assert int(table["count"].sum()) == n and M.table_ok(table, n, int(out[1]))
        assert all(int(f["off"]) % 16 == 0 and int(f["off"]) >= 16 for f in table)
        self.unsplit += int(out[2])
        arena, lens = np.zeros(n * STRIDE, np.uint8), np.zeros(n, np.uint32)
        route.gso_unpack_cpu(self.packed, int(out[1]), table, n, arena, STRIDE, lens)
        for f in table:
            for i in range(int(f["first"]), int(f["first"]) + int(f["count"])):
                pkt = arena[i * STRIDE + 4:i * STRIDE + 4 + int(lens[i])].tobytes()
                if len(pkt) >= 20 and pkt[0] >> 4 == 4 and pkt[9] == self.proto and pkt[16:20] == socket.inet_aton(PEER_IP):
                    self.kinds.append((int(f["kind"]), int(f["count"])))
                    self.packets.append(pkt)
        return n


def test_udp_segment_message_comes_out_as_datagrams():
    """(a) one UDP_SEGMENT message routed into the TUN: a UDP4 super-frame where the queue takes USO, else the
    kernel's own segments with their checksums left partial (CSUM) -- the datagrams are the same."""
    rc, fds, name = route.tun_open_offload(b"qgcmg%d", 1, _lib.TUN_TSO4 | _lib.TUN_USO)
    if rc == 0:
        if _lib.lib().qgcm_tun_up(name, HOST_IP.encode(), 24, 1433) < 0:
            _lib.lib().qgcm_tun_close(fds[0])
            pytest.skip("TUN link set-up refused")
        fd = fds[0]
    else:
        fd = open_tun(_lib.TUN_TSO4)  # a kernel without TUN_F_USO4
    try:
        sk = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
        sk.bind((HOST_IP, 0))
        msg = bytes(np.random.default_rng(0xA).integers(0, 256, 4 * 500 + 123, dtype=np.uint8))
        try:
            sk.sendmsg([msg], [(socket.IPPROTO_UDP, UDP_SEGMENT, struct.pack("H", 500))], 0, (PEER_IP, 9400))
        except OSError as e:
            pytest.skip(f"UDP_SEGMENT refused ({e})")
        finally:
            sk.close()
        r = Reader(fd, 17)
        for _ in range(40):
            if r.read() == 0 and len(r.packets) >= 5:
                break
        assert len(r.packets) == 5
        for pkt in r.packets:
            assert M.verify(pkt) == (True, True) and struct.unpack("!H", pkt[22:24])[0] == 9400
        assert b"".join(p[28:] for p in r.packets) == msg
        assert all(k in (M.UDP4, M.CSUM, M.PLAIN) for k, _ in r.kinds)
    finally:
        _lib.lib().qgcm_tun_close(fd)


def tcp_packet(src, dst, sport, dport, seq, ack, flags, options=b""):
    hl = 20 + len(options)
    t = bytearray(struct.pack("!HHIIBBHHH", sport, dport, seq, ack, (hl // 4) << 4, flags, 65535, 0, 0) + options)
    ip = bytearray(struct.pack("!BBHHHBBH4s4s", 0x45, 0, 20 + hl, 0x4242, 0x4000, 64, 6, 0, socket.inet_aton(src), socket.inet_aton(dst)))
    ip[10:12] = M.rfc1071(bytes(ip)).to_bytes(2, "big")
    pseudo = bytes(ip[12:20]) + bytes([0, 6]) + hl.to_bytes(2, "big")
    t[16:18] = M.rfc1071(pseudo + bytes(t)).to_bytes(2, "big")
    return bytes(ip) + bytes(t)


def test_tcp_sendall_comes_out_as_a_super_frame(tun):
    """(b) a local client's SYN is answered with a hand-built SYN-ACK written to the TUN; what its 12 KiB sendall
    produces is read as TCP4 super-frames, cut, verified and reassembled."""
    client = socket.socket(socket.AF_INET, socket.SOCK_STREAM)
    client.bind((HOST_IP, 0))
    client.setblocking(False)
    try:
        assert client.connect_ex((PEER_IP, 9401)) != 0  # in progress
        r = Reader(tun, 6)
        for _ in range(40):
            r.read()
            if r.packets:
                break
        assert r.packets, "no SYN came out of the TUN"
        syn = r.packets[0]
        assert syn[33] & 0x02 and M.verify(syn) == (True, True)  # the checksum completed where it was left partial
        sport, seq = struct.unpack("!H", syn[20:22])[0], struct.unpack("!I", syn[24:28])[0]
        reply = tcp_packet(PEER_IP, HOST_IP, 9401, sport, 0x1000, (seq + 1) & 0xFFFFFFFF, 0x12, struct.pack("!BBH", 2, 4, 1393))
        assert os.write(tun, bytes(10) + reply) == 10 + len(reply)  # a vnet header of zeros: nothing left to the kernel
        client.setblocking(True)
        client.settimeout(5)
        data = bytes(np.random.default_rng(0xB).integers(0, 256, 12288, dtype=np.uint8))
        client.sendall(data)  # completes the handshake first
        r.kinds, r.packets = [], []
        got = {}
        for _ in range(60):
            r.read()
            for pkt in r.packets:
                hl = 20 + 4 * (pkt[32] >> 4)
                if len(pkt) > hl:
                    assert M.verify(pkt) == (True, True)
                    got[(struct.unpack("!I", pkt[24:28])[0] - seq - 1) & 0xFFFFFFFF] = pkt[hl:]
            r.packets = []
            if sum(len(v) for v in got.values()) >= len(data):
                break
        whole = b"".join(got[k] for k in sorted(got))
        assert whole == data and list(np.cumsum([0] + [len(got[k]) for k in sorted(got)])[:-1]) == sorted(got)
        assert any(k == M.TCP4 and c > 1 for k, c in r.kinds), r.kinds  # a real super-frame, not single packets
        assert r.unsplit == 0
    finally:
        client.close()


def test_arguments_and_the_stop_rules(tun):
    """(c)"""
    L = _lib.lib()
    packed, frames, out = np.zeros(1 << 18, np.uint8), np.zeros(8, M.FRAME), np.zeros(3, np.uint64)
    room = 65536 + 16

    def call(fd=tun, p=packed.ctypes.data, cap=packed.size, f=frames.ctypes.data, mf=8, mn=4096, t=10):
        return L.qgcm_tun_read_gso(fd, p, cap, f, mf, mn, t, out.ctypes.data)

    # the kernel may still send link-up chatter; once the queue stays empty for a 10 ms wait the call times out with 0
    for _ in range(100):
        n = call()
        assert n >= 0
        if n == 0:
            break
    assert n == 0 and out.tolist() == [0, 0, 0]
    assert call(fd=-1) == -1 and call(p=None) == -1 and call(f=None) == -1
    assert call(cap=room - 1) == -1 and call(mn=_lib.GSO_SEGS - 1) == -1
    assert call(mf=0) == 0
    assert L.qgcm_tun_open_offload(b"qgcmg%d", 1, (C_int * 1)(), None, 0, 4) == -22  # an offload bit that is not one
    assert L.qgcm_tun_open_offload(b"qgcmg%d", 0, (C_int * 1)(), None, 0, 1) == -22
    sk = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
    sk.bind((HOST_IP, 0))
    for j in range(4):
        sk.sendto(bytes([j]) * 100, (PEER_IP, 9402))
    sk.close()
    seen = []

    def take(n):
        assert n >= 0 and out[0] == n
        for f in frames[:n]:
            pkt = packed[int(f["off"]):int(f["off"]) + int(f["len"])].tobytes()
            if len(pkt) == 128 and pkt[9] == 17:
                seen.append(pkt[28])
        return n

    assert take(call(cap=room)) == 1                 # room for one read only
    assert take(call(mn=_lib.GSO_SEGS)) == 1           # after one slot fewer than QGCM_GSO_SEGS are left
    assert take(call(mf=1)) == 1
    for _ in range(20):
        if len(seen) == 4 or take(call()) == 0:
            break
    assert seen == [0, 1, 2, 3]

