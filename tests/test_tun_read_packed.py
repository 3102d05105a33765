"""CPU: qgcm_tun_read_packed (quantum_amd/csrc/tun_batch.cpp) on a TUN device, shaped like tests/test_tun_batch.py:
the packets the kernel routes into the device come back to back in a packed area, one qgcm_frame each, every off a
multiple of 16 -- the same packets, in order and byte for byte, as qgcm_tun_read_slots gets.  Needs /dev/net/tun
and CAP_NET_ADMIN; skipped where the kernel refuses."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from quantum_amd import route
from test_tun_batch import HOST_IP, PEER_IP, STRIDE, tun  # noqa: F401  (tun: the fixture)

ROOM = 65536


def send_flow(port, count, size_of=lambda j: 50 + 7 * j, tag=None):
    """One UDP flow (one queue, in order) of `count` datagrams into the device's subnet -> the payloads."""
    sk = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
    sk.bind((HOST_IP, 0))
    sent = [bytes([(port if tag is None else tag) & 255, j & 255]) * ((size_of(j) + 1) // 2) for j in range(count)]
    for msg in sent:
        sk.sendto(msg, (PEER_IP, port))
    sk.close()
    return sent


def ours(pkt: bytes, port: int):
    """The UDP payload of an IPv4 packet of our flow, else None (link-up chatter)."""
    if len(pkt) < 28 or pkt[0] >> 4 != 4 or pkt[9] != 17 or pkt[16:20] != socket.inet_aton(PEER_IP):
        return None
    ihl = (pkt[0] & 15) * 4
    if int.from_bytes(pkt[ihl + 2:ihl + 4], "big") != port:
        return None
    return pkt[ihl + 8:]


def read_packed(fd, packed, max_n, timeout_ms=50):
    frames, out = np.zeros((max(1, max_n), 2), np.uint32), np.full(2, 99, np.uint64)
    n = route.tun_read_packed(fd, packed, frames, max_n, timeout_ms, out)
    assert n >= 0 and out.tolist()[0] == n
    if n:
        assert np.all(frames[:n, 0] % 16 == 0)                                     # every off on its boundary
        ends = frames[:n, 0].astype(np.int64) + frames[:n, 1]
        assert np.all(frames[1:n, 0] == (ends[:-1] + 15) // 16 * 16)               # back to back
        assert int(frames[0, 0]) == 0 and int(out[1]) == int(ends[-1])             # out: the end of the last frame
        assert int(frames[n - 1, 0]) + ROOM <= packed.size                         # read only with the room
    else:
        assert out.tolist() == [0, 0]
    return [packed[o:o + l].tobytes() for o, l in frames[:n].tolist()]


def drain(fds, packed, port, want, max_n=256):
    got = []
    for _ in range(40):
        for fd in fds:
            got += [p for p in (ours(pkt, port) for pkt in read_packed(fd, packed, max_n)) if p is not None]
        if len(got) >= want:
            break
    return got


def test_packed_read_gets_what_the_slot_read_gets(tun):
    """Two flows of the same datagrams, one read packed and one read into slots (a packet can be read only once):
    the same payloads of the same lengths, in order, byte for byte."""
    L, fds, _ = tun
    packed = np.zeros(1 << 20, np.uint8)
    sent = send_flow(9400, 48, tag=0x5A)
    assert drain(fds, packed, 9400, len(sent)) == sent
    sent2 = send_flow(9401, 48, tag=0x5A)
    arena, lens, got = np.zeros(256 * STRIDE, np.uint8), np.zeros(256, np.uint32), []
    for _ in range(40):
        for fd in fds:
            r = L.qgcm_tun_read_slots(fd, arena.ctypes.data, STRIDE, 256, lens.ctypes.data, 50)
            assert r >= 0
            got += [p for p in (ours(bytes(arena[i * STRIDE + 4:i * STRIDE + 4 + lens[i]]), 9401) for i in range(r)) if p is not None]
        if len(got) >= len(sent2):
            break
    assert got == sent2 == sent


def test_it_stops_at_max_n_and_leaves_the_rest_queued(tun):
    L, fds, _ = tun
    packed = np.zeros(1 << 20, np.uint8)
    sent = send_flow(9402, 20)
    got, calls = [], 0
    for _ in range(200):
        for fd in fds:
            pkts = read_packed(fd, packed, 3, timeout_ms=20)
            assert len(pkts) <= 3
            calls += bool(pkts)
            got += [p for p in (ours(pkt, 9402) for pkt in pkts) if p is not None]
        if len(got) >= len(sent):
            break
    assert got == sent and calls >= 7


def test_it_stops_when_under_65536_bytes_of_room_are_left(tun):
    """An area of 65536 + 2000 bytes: after the first packets less than 65536 bytes are left, the call returns
    what it has, and the rest is still queued for the next call."""
    L, fds, _ = tun
    packed = np.zeros(ROOM + 2000, np.uint8)
    sent = send_flow(9403, 12, size_of=lambda j: 1000)
    got, sizes = [], []
    for _ in range(200):
        for fd in fds:
            mine = [p for p in (ours(pkt, 9403) for pkt in read_packed(fd, packed, 256, timeout_ms=20)) if p is not None]
            if mine:
                sizes.append(len(mine))
            got += mine
        if len(got) >= len(sent):
            break
    assert got == sent
    # a frame of 1028 bytes takes 1040 of the area: the second may start at 1040 <= 2000, a third at 2080 may not
    # (other traffic of the link only shortens a call's share)
    assert max(sizes) <= 2 and len(sizes) >= 6, sizes


def test_timeout_and_bad_arguments(tun):
    L, fds, _ = tun
    packed, frames, out = np.zeros(ROOM, np.uint8), np.zeros((4, 2), np.uint32), np.zeros(2, np.uint64)
    for _ in range(100):  # link-up chatter first; then the queue stays empty
        r = L.qgcm_tun_read_packed(fds[0], packed.ctypes.data, packed.size, frames.ctypes.data, 4, 10, out.ctypes.data)
        assert r >= 0
        if r == 0:
            break
    assert r == 0 and out.tolist() == [0, 0]
    out[:] = 7
    assert L.qgcm_tun_read_packed(-1, packed.ctypes.data, packed.size, frames.ctypes.data, 4, 0, out.ctypes.data) == -1
    assert out.tolist() == [0, 0]
    assert L.qgcm_tun_read_packed(fds[0], None, packed.size, frames.ctypes.data, 4, 0, None) == -1
    assert L.qgcm_tun_read_packed(fds[0], packed.ctypes.data, packed.size, None, 4, 0, None) == -1
    assert L.qgcm_tun_read_packed(fds[0], packed.ctypes.data, ROOM - 1, frames.ctypes.data, 4, 0, None) == -1
    assert L.qgcm_tun_read_packed(fds[0], packed.ctypes.data, packed.size, frames.ctypes.data, 0, 0, None) == 0
    assert L.qgcm_tun_read_packed(fds[0], packed.ctypes.data, packed.size, frames.ctypes.data, 4, 0, None) == 0  # out NULL


@pytest.mark.parametrize("mode", ["-1", "1"])
def test_the_other_read_modes(mode):
    """poll + read per packet (QGCM_TUN_URING=-1) and, with QGCM_TUN_URING=1, still preadv2 -- each in a fresh
    process: the form is fixed at a process's first batched read."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, QGCM_TUN_URING=mode)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider",
                        os.path.join(root, "tests", "test_tun_read_packed.py"), "-k", "stops_at_max_n or stops_when_under"],
                       cwd=root, env=env, capture_output=True, text=True, timeout=120)
    if "skipped" in r.stdout and "passed" not in r.stdout:
        pytest.skip("TUN device refused in the child")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "2 passed" in r.stdout, r.stdout[-1000:]
