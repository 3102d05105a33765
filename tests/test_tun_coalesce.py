"""CPU: qgcm_tun_write_gso on a real TUN queue with IFF_VNET_HDR.  The test listens on a TCP socket on the TUN's
address and plays the remote peer through the queue: a hand-built SYN, the SYN-ACK read back, an ACK, then 12 KiB as
one coalesced entry that qgcm_deliver_coalesce_cpu made of 1348-byte segments; recv returns the 12 KiB, so the kernel
took the vnet header and the partial checksum.  A PLAIN UDP datagram goes through the same call.  Needs
/dev/net/tun and CAP_NET_ADMIN; skipped where the device or the link set-up is refused, or no SYN-ACK answers.  No
entry may fall back to the host segmentation: the fall-back has the sanitizer driver's socketpair for its test."""
import socket
import struct

import numpy as np
import pytest

import coalesce_model as M
from quantum_amd import _lib, route
from test_tun_gso import tcp_packet

HOST_IP, PEER_IP = "10.213.11.1", "10.213.11.2"  # a subnet of this file's own
STRIDE = 1536


def read_packets(fd):
    """one qgcm_tun_read_gso, cut by qgcm_gso_unpack_cpu -> the packets as bytes"""
    packed, frames, out = np.zeros(1 << 18, np.uint8), np.zeros(16, M.GSO_FRAME), np.zeros(3, np.uint64)
    n = route.tun_read_gso(fd, packed, frames, 8192, 50, out)
    if n <= 0:
        return []
    arena, lens = np.zeros(n * STRIDE, np.uint8), np.zeros(n, np.uint32)
    route.gso_unpack_cpu(packed, int(out[1]), frames[:int(out[0])], n, arena, STRIDE, lens)
    return [arena[i * STRIDE + 4:i * STRIDE + 4 + int(lens[i])].tobytes() for i in range(n)]


def be(ip):
    return int.from_bytes(socket.inet_aton(ip), "big")


@pytest.fixture(params=(0, _lib.TUN_TSO4), ids=("no_offloads", "tso4"))
def tun(request):
    rc, fds, name = route.tun_open_offload(b"qgcmc%d", 1, request.param)
    if rc < 0:
        pytest.skip(f"offload TUN refused (errno {-rc})")
    if _lib.lib().qgcm_tun_up(name, HOST_IP.encode(), 24, 1433) < 0:
        _lib.lib().qgcm_tun_close(fds[0])
        pytest.skip("TUN link set-up refused")
    yield fds[0]
    _lib.lib().qgcm_tun_close(fds[0])


def coalesced(f, n):
    arena, lens = M.build(f, STRIDE, np.random.default_rng(0xC))
    packed = np.zeros(n * (STRIDE + 16), np.uint8)
    frames, counts = route.deliver_coalesce_cpu(arena, STRIDE, n, lens, np.zeros(n, np.uint32), None, packed)
    return arena, packed, frames, counts


def test_twelve_kib_go_up_as_one_coalesced_entry(tun):
    srv = socket.socket(socket.AF_INET, socket.SOCK_STREAM)
    srv.setsockopt(socket.SOL_SOCKET, socket.SO_REUSEADDR, 1)
    try:
        srv.bind((HOST_IP, 0))
        srv.listen(1)
        srv.settimeout(5)
        port, sport, isn = srv.getsockname()[1], 40123, 0x7000
        syn = tcp_packet(PEER_IP, HOST_IP, sport, port, isn, 0, 0x02, struct.pack("!BBH", 2, 4, 1393))
        one = np.zeros(1, M.GSO_FRAME)

        def write_plain(pkt):
            buf = np.zeros(16 + len(pkt), np.uint8)
            buf[16:] = np.frombuffer(pkt, np.uint8)
            one[0] = (16, len(pkt), 0, 1, 0, 0, 0, 0, M.PLAIN, 0)
            return route.tun_write_gso(tun, buf, buf.size, one)

        assert write_plain(syn) == 1
        synack = []
        for _ in range(40):
            synack = [p for p in read_packets(tun) if len(p) >= 40 and p[9] == 6 and p[33] == 0x12 and
                      p[16:20] == socket.inet_aton(PEER_IP)]
            if synack:
                break
        if not synack:
            pytest.skip("no SYN-ACK came out of the TUN")
        their = struct.unpack("!I", synack[0][24:28])[0]
        ack = (their + 1) & 0xFFFFFFFF
        assert write_plain(tcp_packet(PEER_IP, HOST_IP, sport, port, isn + 1, ack, 0x10)) == 1
        conn, _ = srv.accept()
        conn.settimeout(5)
        # 12 KiB in 1348-byte segments: nine, and a tail of 156 that joins them
        sizes = [1348] * 9 + [12288 - 9 * 1348]
        n = len(sizes)
        f = M.fields(n)
        M.run(f, 0, n, sizes, seq0=isn + 1, id0=0x4243)
        f["src"][:], f["dst"][:], f["sport"][:], f["dport"][:], f["ack"][:], f["win"][:] = be(PEER_IP), be(HOST_IP), sport, port, ack, 65535
        f["flags"][n - 1] = M.ACK | M.PSH
        arena, packed, frames, counts = coalesced(f, n)
        assert tuple(counts) == (1, 16 + ((40 + 12288 + 15) & ~15), 1, n) and frames[0]["kind"] == M.TCP4
        out = np.zeros(3, np.uint64)
        assert route.tun_write_gso(tun, packed, int(counts[1]), frames, out) == 1
        assert out.tolist() == [1, n, 0]  # the kernel took the super-frame itself: nothing fell back
        got = b""
        while len(got) < 12288:
            piece = conn.recv(65536)
            assert piece
            got += piece
        rows = arena.reshape(n, STRIDE)
        assert got == b"".join(rows[i, 44:44 + sizes[i]].tobytes() for i in range(n))
        # the peer resets, so that the connection leaves nothing behind that retransmits
        assert write_plain(tcp_packet(PEER_IP, HOST_IP, sport, port, (isn + 1 + 12288) & 0xFFFFFFFF, ack, 0x14)) == 1
        conn.close()
    finally:
        srv.close()


def test_a_plain_udp_datagram_goes_through_the_same_call(tun):
    sk = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
    try:
        sk.bind((HOST_IP, 0))
        sk.settimeout(5)
        port = sk.getsockname()[1]
        payload = bytes(np.random.default_rng(0xD).integers(0, 256, 333, dtype=np.uint8))
        udp = bytearray(struct.pack("!HHHH", 9403, port, 8 + len(payload), 0) + payload)
        ip = bytearray(struct.pack("!BBHHHBBH4s4s", 0x45, 0, 20 + len(udp), 1, 0x4000, 64, 17, 0, socket.inet_aton(PEER_IP),
                                   socket.inet_aton(HOST_IP)))
        from gso_model import rfc1071
        ip[10:12] = rfc1071(bytes(ip)).to_bytes(2, "big")
        udp[6:8] = (rfc1071(bytes(ip[12:20]) + bytes([0, 17]) + len(udp).to_bytes(2, "big") + bytes(udp)) or 0xFFFF).to_bytes(2, "big")
        pkt = np.frombuffer(bytes(ip) + bytes(udp), np.uint8)
        # through the coalescing: one PLAIN entry
        arena = np.zeros(STRIDE, np.uint8)
        arena[4:4 + len(pkt)] = pkt
        packed = np.zeros(STRIDE + 16, np.uint8)
        frames, counts = route.deliver_coalesce_cpu(arena, STRIDE, 1, np.array([len(pkt)], np.uint32), np.zeros(1, np.uint32), None, packed)
        assert tuple(counts) == (1, 16 + ((len(pkt) + 15) & ~15), 0, 1) and frames[0]["kind"] == M.PLAIN
        out = np.zeros(3, np.uint64)
        assert route.tun_write_gso(tun, packed, int(counts[1]), frames, out) == 1
        assert out.tolist() == [1, 1, 0]
        data, src = sk.recvfrom(4096)
        assert data == payload and src == (PEER_IP, 9403)
    finally:
        sk.close()
