"""Batches of the coalescing tests (CPU and GPU), built with tests/coalesce_model.py's builder: the one-rule-broken
runs with the frame starts the contract gives them, and the mixed batch that holds every case at once."""
import numpy as np

import coalesce_model as M

SENTINEL = 0xA5


class Batch:
    """field arrays that grow run by run, then edits applied to the built arena"""

    def __init__(self, stride):
        self.stride, self.parts, self.edits, self.n = stride, [], [], 0
        self.status, self.peer = [], []

    def room(self, hdr=40):
        return self.stride - 4 - hdr

    def run(self, count, P, status=1, peer=7, **kw):
        f = M.fields(count)
        M.run(f, 0, count, P, **kw)
        self.parts.append(f)
        self.status += [status] * count
        self.peer += [peer] * count
        lo, self.n = self.n, self.n + count
        return lo

    def edit(self, fn):
        """fn(arena, lens) after the build"""
        self.edits.append(fn)

    def done(self, seed=1):
        f = {k: np.concatenate([p[k] for p in self.parts]) for k in self.parts[0]}
        arena, lens = M.build(f, self.stride, np.random.default_rng(seed))
        for fn in self.edits:
            fn(arena, lens)
        return arena, lens, np.array(self.peer, np.uint32), np.array(self.status, np.uint8)


# (name, what differs from slot 3 on / at slot 3 of a run of six, the frame starts that result)
def split_cases():
    def field(name, value, only=False):
        def apply(b, lo):
            f = b.parts[-1]
            if only:
                f[name][3] = value
            else:
                f[name][3:] = value
        return apply

    def flip_payload(b, lo):
        b.edit(lambda arena, lens: arena.__setitem__((lo + 3) * b.stride + 4 + 40 + 5, arena[(lo + 3) * b.stride + 4 + 40 + 5] ^ 0x10))

    def bad_ip_csum(b, lo):
        b.edit(lambda arena, lens: arena.__setitem__((lo + 3) * b.stride + 4 + 10, arena[(lo + 3) * b.stride + 4 + 10] ^ 0x01))

    def id_gap(b, lo):
        b.parts[-1]["id"][3:] += 1

    def seq_gap(b, lo):
        b.parts[-1]["seq"][3:] += 1

    def opt_byte(b, lo):  # a TCP option byte (the runs with options have doff 32)
        def go(arena, lens):
            for s in range(lo + 3, lo + 6):
                arena[s * b.stride + 4 + 20 + 24] ^= 0x40
            M.fix_checksums(arena, b.stride, np.arange(lo + 3, lo + 6), lens)
        b.edit(go)

    def peer(b, lo):
        b.peer[lo + 3:lo + 6] = [8, 8, 8]

    def dropped(b, lo):
        b.status[lo + 3] = 0

    def too_long(b, lo):  # status 1 with 4 + L > stride
        b.edit(lambda arena, lens: lens.__setitem__(lo + 3, b.stride - 3))

    def flag(bit):
        return field("flags", M.ACK | bit, only=True)

    return [
        ("payload bit", flip_payload, (0, 3, 4)), ("ip checksum", bad_ip_csum, (0, 3, 4)), ("id gap", id_gap, (0, 3)),
        ("seq gap", seq_gap, (0, 3)), ("ack", field("ack", 77), (0, 3)), ("window", field("win", 513), (0, 3)),
        ("ttl", field("ttl", 63), (0, 3)), ("tos", field("tos", 8), (0, 3)), ("option byte", opt_byte, (0, 3)),
        ("peer", peer, (0, 3)), ("psh in the middle", lambda b, lo: b.parts[-1]["flags"].__setitem__(2, M.ACK | M.PSH), (0, 3)),
        ("fin", flag(M.FIN), (0, 3, 4)), ("syn", flag(M.SYN), (0, 3, 4)), ("rst", flag(M.RST), (0, 3, 4)),
        ("urg", flag(M.URG), (0, 3, 4)), ("ece", flag(M.ECE), (0, 3, 4)),
        ("fragment", field("frag", 0x2000, only=True), (0, 3, 4)), ("fragment offset", field("frag", 0x4001, only=True), (0, 3, 4)),
        ("reserved bit", field("frag", 0x8000, only=True), (0, 3, 4)), ("df differs", field("frag", 0), (0, 3)),
        ("dropped slot", dropped, (0, 4)), ("too long for the slot", too_long, (0, 4)),
    ]


def add_split(b, case, P=24, flow=0):
    """a run of six with `case` applied; -> its first slot"""
    lo = b.run(6, P, flow=flow, doff=32, seq0=5000 + 977 * flow, id0=100 * flow)
    case[1](b, lo)
    return lo


def zero_checksum(b, slot, field):
    """the TCP checksum of `slot` (ihl 20) recomputes to 0x0000 after a payload word took the old field's value in;
    the field is then set to `field`: 0x0000 is what is recomputed, 0xffff sums right too but is no candidate"""
    def go(arena, lens):
        at = slot * b.stride + 4
        old = int(arena[at + 36]) << 8 | int(arena[at + 37])
        s = (int(arena[at + 40]) << 8 | int(arena[at + 41])) + old
        s = (s & 0xFFFF) + (s >> 16)
        arena[at + 40], arena[at + 41], arena[at + 36], arena[at + 37] = s >> 8, s & 255, field >> 8, field & 255
    b.edit(go)


def ip_option_differs(b, lo, count, since):
    """an IP option byte (ihl 28) differs from slot lo + since on, checksums right"""
    def go(arena, lens):
        slots = np.arange(lo + since, lo + count)
        arena[slots * b.stride + 4 + 22] ^= 0x40
        M.fix_checksums(arena, b.stride, slots, lens)
    b.edit(go)


def mixed(stride, seed=3):
    """-> (arena, lens, peer, status): runs that straddle slots 63/64 and 255/256, every P residue mod 16, ihl and doff
    across 20..60, every split rule, both cuts, the tails, the wraps, drops, misses, empty, short and non-TCP packets"""
    b = Batch(stride)
    P = min(1348, b.room())
    b.run(70, P, flow=1)                                     # 0..69: the cut at 64 members, across 63/64
    b.run(3, 9, flow=2, proto=17)                            # non-TCP
    b.run(2, 30, flow=3, status=0)                           # dropped
    b.run(2, 30, flow=3, status=2)                           # a miss
    for r in range(16):                                      # every P residue mod 16
        b.run(3, 32 + r, flow=10 + r, seq0=0xFFFFFFFF - 40, id0=0xFFFE)   # ... across the seq and id wraps
    for i, ihl in enumerate(range(20, 64, 4)):
        for doff in (20, 32, 60):
            b.run(3, min(50, b.room(ihl + doff)), flow=40 + i, ihl=ihl, doff=doff)
    while b.n < 250:
        b.run(1, 5 + b.n % 7, flow=b.n)                      # lone packets of other flows
    b.run(12, min(1000, b.room()), flow=4)                   # 250..261: across 255/256
    for i, case in enumerate(split_cases()):
        add_split(b, case, P=17 + i, flow=100 + i)
    if b.room() >= 1100:
        b.run(130, 1100, flow=5)                             # the cut at 65535 bytes: m = 59
    q = min(40, b.room())
    b.run(4, [q, q, q, q - 3], flow=6)                       # a tail
    b.run(65, [20] * 64 + [7], flow=7)                       # a full frame, then no tail
    b.run(3, [q, q - 1, q - 2], flow=8)                      # three falling sizes
    b.run(4, [q, q - 5, q - 5, q - 5], flow=9)               # a tail that is followed by an eq pair is none
    b.run(3, [q, q, q + 1], flow=10)                         # a longer one never joins
    lo = b.run(4, 33, flow=11)
    b.parts[-1]["flags"][3] = M.ACK | M.PSH                  # PSH on the last member
    lo = b.run(3, 12, flow=12)
    b.edit(lambda arena, lens, lo=lo: lens.__setitem__(lo + 1, 0))    # an empty packet
    lo = b.run(2, 12, flow=13)
    b.edit(lambda arena, lens, lo=lo: lens.__setitem__(lo, 39))       # too short for a candidate
    for field in (0x0000, 0xFFFF):                           # recomputed 0x0000: the field 0x0000 merges, 0xffff does not
        zero_checksum(b, b.run(3, 30, flow=15) + 1, field)
    ip_option_differs(b, b.run(6, 19, flow=16, ihl=28), 6, 3)
    rng = np.random.default_rng(seed)
    while b.n < 2300:                                        # trains of every length and size, one in ten dropped
        ihl, doff = int(rng.choice((20, 20, 20, 28))), int(rng.choice((20, 32)))
        b.run(int(rng.integers(1, 12)), int(rng.integers(1, min(1400, b.room(ihl + doff)) + 1)), flow=b.n,
              status=int(rng.random() >= 0.1), ihl=ihl, doff=doff)
    while b.n % 256 != 255:
        b.run(1, 6, flow=b.n)
    b.run(5, min(333, b.room()), flow=14, peer=9)            # across a scan tile's edge once more
    return b.done(seed)


def trains(n, stride, P, segs, seed=5, drop=0.0):
    """n slots of `segs`-segment trains of payload P (a number, or (lo, hi) for a random size per train), a fraction
    `drop` of the slots dropped: the large batches"""
    rng = np.random.default_rng(seed)
    f = M.fields(n)
    k = np.arange(n)
    train, at = k // segs, k % segs
    size = np.full(n, P) if np.isscalar(P) else rng.integers(P[0], P[1] + 1, n // segs + 1)[train]
    f["P"] = size.astype(np.int64)
    f["seq"] = (7 + 100003 * train + at * size) & 0xFFFFFFFF
    f["id"] = (train * 31 + at) & 0xFFFF
    f["sport"] = 1024 + train % 50000
    arena, lens = M.build(f, stride, rng)
    status = (rng.random(n) >= drop).astype(np.uint8)
    return arena, lens, np.full(n, 3, np.uint32), status
