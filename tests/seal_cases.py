"""Records to seal, for every seal path: the generator (numpy and the oracle only; no GPU, no torch).

The sibling of forgery_cases.py.  A batch is an arena of slots in which EVERY byte is random before the
seal: headers, payloads, the 28 bytes where tag and nonce will go, the gap behind each record, the lead
before slot 0 and a few bytes behind the last slot.  A seal that writes one byte past its record, or that
does not put back a gap byte it staged, so differs from the oracle, whatever value it writes.  Slots keep
no room behind the record: at the minimal stride a record's last dword touches the next slot's header.

What a seal must leave behind is never worked out here and never by the code under test: `oracle_seal`
runs O.aesgo_seal_descs on a copy of the arena; `openssl_seal` is the independent second opinion
(test_seal_cases.py holds the two together over the whole matrix).  Every packet of the matrix is valid:
rejected packets belong to test_gpu_desc_edges.py.

The nonce comes from an array of 12 bytes a packet, or (`nonces` None) from the slot: the random 12 bytes
already at [4 + L + 16, 4 + L + 28).

Why these lengths (quantum_amd/csrc/gcm_kernels.hip):
  quad_packet branches on nfull & 3 (the lane that owns the partial block), d & 3 (the lane whose spare
  AES slot computes E_K(J0)), L & 15 (the words and bytes of the partial block, the prefix handed to
  write_tail) and L & 3 (the funnel shifts of write_tail, the byte loads of read_nonce): L mod 64, and
  0..130 visits every residue twice, lanes that own no block (d <= 3) included.  16 k and 16 k + 1,
  k = 9..67, give every block count up to 68 and every GHASH exponent count up to 70 (one_packet's
  `ntabs` changes at emax = d + 2 = 2, 4, 8, 16, 32 and 64, i.e. behind L = 0, 32, 96, 224, 480 and 992).
  With at most 4 bytes of additional data (na = 1) one_packet's flat GHASH holds while d + 2 <= 128
  (L <= 2016), its column-sliced counter pass while d + 1 <= 128 (L <= 2032); 2048 is the next block.
  Counter block 254 (L 4049..4064) is the first whose counter has a second byte, 255 and 256 follow, and
  8192 is block 512.  4 + L + 28 = 8192 at L = 8160 fills one_packet's staging rows 0..511, one a thread;
  a byte more starts the second row a thread (rows tid + 512 k, k < 4: 32 KiB, the whole staging area).
  L = 32720 is the longest record the one-workgroup kernel stages; 32721 goes to the quad kernel.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from oracle import oracle as O

OVERHEAD = 28  # tag 16 + nonce 12
TRAIL = 32  # random bytes behind the last slot: the allocation's end, compared like every gap

NKEYS = 32
KEYS = np.random.default_rng(0x5EA1CA5E).bytes(32 * NKEYS)

SHORT = tuple(range(131))
SERIES = tuple(16 * k + j for k in range(9, 68) for j in (0, 1))
ONE_EDGES = tuple(e + j for e in (2016, 2032, 2048) for j in (-1, 0, 1))
MTU = (1349, 1350, 1351, 1353, 1433)
COUNTER = tuple(e + j for e in (4048, 4064, 4080, 4096, 8192) for j in (-1, 0, 1))
STAGING = (8159, 8160, 8161)
JUMBO = (9000,)
CAP = (32719, 32720, 32721)  # sealed three packets at a time
SEAL_LENGTHS = tuple(sorted(set(SHORT + SERIES + ONE_EDGES + MTU + COUNTER + STAGING + JUMBO + CAP)))
DESC_LENGTHS = tuple(L for L in SEAL_LENGTHS if L < 9001)  # the descriptor batches leave the cap lengths out
ONE_CAP_LEN = CAP[1]

# plain numbers, asserted by test_seal_cases.py: a generator that silently makes fewer cases fails
COUNTS = {"lengths": 285, "desc_lengths": 282, "quad_packets": 37 * 282 + 3 * 3, "one_packets": 5 * 282 + 3 * 2,
          "per_wave": 282, "segmented": 753 + 131, "descs_one": 131 + 9, "per_packet": 9 + 118}

STRIDES = {
    "min4": lambda L: (4 + L + OVERHEAD + 3) & ~3,  # the smallest run_uniform takes: slots walk through every offset mod 16
    "s16": lambda L: (4 + L + OVERHEAD + 15) & ~15,  # = batch.slot_stride(L, 16), the one-workgroup kernel's staging area
    "s16p16": lambda L: ((4 + L + OVERHEAD + 15) & ~15) + 16,
    "s64p4": lambda L: ((4 + L + OVERHEAD + 63) & ~63) + 4,  # batch.slot_stride(L, 64) + 4
}

# the uniform quad kernel's four configurations: (lead, stride class, nonce from the slot)
QUAD_CONFIGS = {"s16_array": (0, "s16", False), "min4_slot": (60, "min4", True), "min4_array": (0, "min4", False),
                "s64p4_slot": (60, "s64p4", True)}
QUAD_N, ONE_N, CAP_N = 37, 5, 3  # 37: two full 16-packet tiles and five packets of a third
SEG_MIN_PACKETS = 753  # (kSegMinTiles - 1) * 16 + 1: a key with this many packets is a segmented-kernel run


@dataclass
class Batch:
    arena: np.ndarray  # uint8: lead, slots and trail BEFORE the seal, every byte random
    offs: np.ndarray  # uint64: offset of each slot (Raw[0]) in the arena
    lens: np.ndarray  # uint32: payload length L of each packet
    kidx: np.ndarray  # uint32: key slot of each packet
    size: np.ndarray  # int64: bytes of each slot, gap included
    nonces: np.ndarray | None  # uint8, 12 a packet; None: the nonce is the 12 bytes already in the slot
    keys: bytes  # the key table kidx indexes (32 bytes a slot)
    aad_len: int
    stride: int  # the uniform stride, 0 for packed slots
    lead: int  # bytes before slot 0

    @property
    def n(self) -> int:
        return len(self.offs)

    @property
    def end(self) -> int:
        """The end of the last slot; TRAIL more bytes follow."""
        return int(self.offs[-1] + self.size[-1])

    def slot_nonces(self) -> np.ndarray:
        """The 12 bytes at [4 + L + 16, 4 + L + 28) of every slot, as they are before the seal."""
        at = (self.offs.astype(np.int64) + 4 + self.lens.astype(np.int64) + 16)[:, None] + np.arange(12)
        return np.ascontiguousarray(self.arena[at].reshape(-1))

    def describe(self, i: int) -> str:
        o = int(self.offs[i])
        return f"packet {i} at {o} ({o % 16} mod 16): L={int(self.lens[i])}, key {int(self.kidx[i])}"


def _finish(rng, offs, lens, kidx, size, from_slot, keys, aad_len, stride, lead) -> Batch:
    n = len(offs)
    arena = rng.integers(0, 256, int(offs[-1] + size[-1]) + TRAIL, dtype=np.uint8)
    nonces = None if from_slot else rng.integers(0, 256, 12 * n, dtype=np.uint8)
    return Batch(arena, np.asarray(offs, np.uint64), np.asarray(lens, np.uint32), np.asarray(kidx, np.uint32),
                 np.asarray(size, np.int64), nonces, keys, aad_len, stride, lead)


def uniform(L: int, n: int, lead: int, stride, from_slot: bool, aad_len: int = 4, key: int = 5, keys: bytes = KEYS,
            seed: int = 0) -> Batch:
    """n slots of one length and key, `stride` (a class of STRIDES, or bytes) apart, slot 0 at `lead`."""
    stride = STRIDES[stride](L) if isinstance(stride, str) else int(stride)
    assert n > 0 and lead % 4 == 0 and stride % 4 == 0 and stride >= 4 + L + OVERHEAD
    rng = np.random.default_rng([0x5EA1, seed, L, n, lead, stride, int(from_slot), aad_len])
    offs = lead + stride * np.arange(n, dtype=np.int64)
    return _finish(rng, offs, np.full(n, L), np.full(n, key), np.full(n, stride), from_slot, keys, aad_len, stride, lead)


def packed(lengths, kidx, from_slot: bool, aad_len: int = 4, base: int = 0, align: int = 4, keys: bytes = KEYS,
           seed: int = 0) -> Batch:
    """One slot a length, packed at `align` with a random gap of 0..2 units behind each record, slot 0 at
    `base` (4 puts align-16 records at 4 mod 16)."""
    assert len(lengths) == len(kidx) > 0 and align % 4 == 0 and base % 4 == 0
    rng = np.random.default_rng([0x5EA1D, seed, len(lengths), int(from_slot), aad_len, base, align])
    L = np.asarray(lengths, np.int64)
    size = (4 + L + OVERHEAD + align - 1) // align * align + align * rng.integers(0, 3, len(L))
    offs = base + np.concatenate([[0], np.cumsum(size)[:-1]])
    return _finish(rng, offs, L, kidx, size, from_slot, keys, aad_len, 0, base)


def on_keys(count: int, key_slots) -> np.ndarray:
    """Key slots for `count` packets, dealt round-robin over key_slots."""
    ks = np.asarray(list(key_slots), np.uint32)
    return ks[np.arange(count) % len(ks)]


def _nonces(b: Batch) -> np.ndarray:
    return b.slot_nonces() if b.nonces is None else b.nonces


def oracle_seal(b: Batch, threads: int = 8):
    """What a seal of the batch must leave: (status, arena), the arena as O.aesgo_seal_descs leaves it.  The
    status array is junk (0x5A) before the call on both sides; every packet is valid and sealed."""
    exp = b.arena.copy()
    O.aesgo_seal_descs(b.keys, exp, b.offs, b.lens, b.kidx, _nonces(b), b.aad_len, threads)
    return np.ones(b.n, dtype=np.uint8), exp


def openssl_seal(b: Batch, threads: int = 8) -> np.ndarray:
    """The same seal by OpenSSL's EVP interface, for test_seal_cases.py."""
    exp = b.arena.copy()
    O.ossl_seal_descs(b.keys, exp, b.offs, b.lens, b.kidx, _nonces(b), b.aad_len, threads)
    return exp


def mismatches(b: Batch, status, arena, want_status, want_arena, limit: int = 6) -> str:
    """'' when status (None: the call had no status array) and arena equal the oracle's, else the first
    packets that differ: index, offset mod 16, length and the first differing byte of the slot."""
    arena = np.asarray(arena)
    st_ok = status is None or np.array_equal(np.asarray(status), want_status)
    if st_ok and np.array_equal(arena, want_arena):
        return ""
    out = []
    for i in range(b.n):
        o, z = int(b.offs[i]), int(b.size[i])
        st = status is not None and int(status[i]) != int(want_status[i])
        diff = np.flatnonzero(arena[o:o + z] != want_arena[o:o + z])
        if st or len(diff):
            L = int(b.lens[i])
            msg = b.describe(i)
            if st:
                msg += f": status {int(status[i])} (oracle {int(want_status[i])})"
            if len(diff):
                at = int(diff[0])
                part = ("header" if at < 4 else "ciphertext" if at < 4 + L else "tag" if at < 4 + L + 16 else
                        "nonce" if at < 4 + L + OVERHEAD else "gap")
                msg += (f": {len(diff)} bytes differ from slot byte {at} ({part}): "
                        f"{int(arena[o + at]):#04x}, oracle {int(want_arena[o + at]):#04x}")
            out.append(msg)
            if len(out) == limit:
                break
    if not np.array_equal(arena[:b.lead], want_arena[:b.lead]):
        out.append("bytes before the first slot differ")
    if not np.array_equal(arena[b.end:], want_arena[b.end:]):
        out.append("bytes behind the last slot differ")
    total = 0 if status is None else int((np.asarray(status) != want_status).sum())
    return f"{total} statuses differ; first packets: " + "; ".join(out)


# ---------------- the matrices the tests use ----------------

def quad_case(L: int, config: str, aad_len: int = 4) -> Batch:
    """One uniform call for the quad kernel: 37 packets (3 at the cap lengths) in a layout of QUAD_CONFIGS."""
    lead, stride, from_slot = QUAD_CONFIGS[config]
    return uniform(L, CAP_N if L >= CAP[0] else QUAD_N, lead, stride, from_slot, aad_len)


def one_case(L: int, stride: str, from_slot: bool, aad_len: int = 4) -> Batch:
    """One uniform call the default dispatch hands to the one-workgroup kernel: 5 packets (3 at the cap
    lengths), 16-B-aligned slots of a 16-B-aligned arena."""
    assert stride in ("s16", "s16p16") and L <= ONE_CAP_LEN
    return uniform(L, CAP_N if L >= CAP[0] else ONE_N, 0, stride, from_slot, aad_len)


def per_wave_case(from_slot: bool, aad_len: int = 4) -> Batch:
    """Every length below 9001 once, over five keys, records 4-B packed from offset 4."""
    return packed(DESC_LENGTHS, on_keys(len(DESC_LENGTHS), [2, 3, 5, 7, 11]), from_slot, aad_len, base=4, seed=1)


def segmented_case(from_slot: bool) -> Batch:
    """The lengths below 9001, cycled, on ONE key until it has 753 packets (a run of the segmented kernel),
    and 0..130 over 16 keys too short for a run (its per-wave pass), shuffled together."""
    run = [DESC_LENGTHS[i % len(DESC_LENGTHS)] for i in range(SEG_MIN_PACKETS)]
    L = np.array(run + list(SHORT))
    kidx = np.concatenate([np.full(len(run), 8, np.uint32), on_keys(len(SHORT), range(9, 25))])
    order = np.random.default_rng(0x5E6).permutation(len(L))
    return packed(L[order], kidx[order], from_slot, 4, base=4, seed=2)


def descs_one_case(from_slot: bool) -> Batch:
    """0..130 and the one-kernel boundaries over three keys, 16-B-aligned records."""
    L = SHORT + ONE_EDGES
    return packed(L, on_keys(len(L), [1, 2, 3]), from_slot, 4, base=0, align=16, seed=3)


PER_PACKET_LENGTHS = ONE_EDGES + SERIES


def all_batches():
    """(name, batch) for every batch the GPU tests seal, for the CPU cross-checks."""
    for config in QUAD_CONFIGS:
        for L in SEAL_LENGTHS:
            yield f"quad {config} L={L}", quad_case(L, config)
    for aad_len in (0, 1, 3):
        for L in SHORT:
            yield f"quad min4_slot aad {aad_len} L={L}", quad_case(L, "min4_slot", aad_len)
    for stride in ("s16", "s16p16"):
        for from_slot in (False, True):
            for L in SEAL_LENGTHS:
                if L <= ONE_CAP_LEN:
                    yield f"one {stride} slot={from_slot} L={L}", one_case(L, stride, from_slot)
    for name in DISPATCH:
        yield f"dispatch {name}", dispatch_case(name)
    for from_slot in (False, True):
        for aad_len in (4, 0):
            yield f"per_wave slot={from_slot} aad {aad_len}", per_wave_case(from_slot, aad_len)
        yield f"segmented slot={from_slot}", segmented_case(from_slot)
        yield f"descs_one slot={from_slot}", descs_one_case(from_slot)


# Uniform calls the default dispatch must hand to the quad kernel, one per reason its predicate (run_uniform)
# refuses the one-workgroup kernel, and two batches past its 2048 packets: (L, n, lead, stride, from_slot)
DISPATCH = {
    "stride_not_16": (17, ONE_N, 0, "min4", False),
    "stride_not_16_mtu": (1351, ONE_N, 0, "min4", True),
    "lead_4": (17, ONE_N, 4, "s16", True),
    "lead_4_mtu": (1351, ONE_N, 4, "s16", False),
    "past_cap": (CAP[2], CAP_N, 0, "s16", False),
    "n2049_L17": (17, 2049, 0, "min4", True),
    "n2049_L1351": (1351, 2049, 0, "min4", True),
}


def dispatch_case(name: str) -> Batch:
    L, n, lead, stride, from_slot = DISPATCH[name]
    assert stride != "min4" or STRIDES["min4"](L) % 16  # a minimal stride that is no multiple of 16
    return uniform(L, n, lead, stride, from_slot)
