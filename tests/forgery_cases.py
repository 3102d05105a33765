"""Forged records for the open paths: the generator (numpy and the oracle only; no GPU, no torch).

A batch is an arena of slots.  Even slots hold authentic records, every one with its own plaintext,
header and nonce; odd slots hold forged ones, each a copy of one authentic base record (one per key and
length) with exactly ONE forgery applied.  A forged packet so sits between two authentic packets that
differ from each other: a status written to the neighbour's index, a zeroing store that spills and a
verdict shared across a quad or a tile all show.  Every slot ends in random gap bytes, and callers
compare the whole arena.

Base records are sealed by the oracle (O.aesgo_seal_descs).  What an open must leave behind is never
worked out here and never by the code under test: `oracle_open` runs O.aesgo_open_descs on a copy of
the arena.

Forgery kinds (`Spec.kind`):
  bit       every single-bit flip of the record [0, 4 + L + 28)            (`bit_specs`)
  bit_long  header, tag and nonce bits, ciphertext edges, a bit per block  (`bit_long_specs`)
  residue   one tag bit for every L = 16 k + r, r = 0..15, k = 0..5        (`residue_specs`)
  field     tag all zero / all ones, tag, nonce or ciphertext of another
            authentic record of the same key and length                    (`field_specs`)
  key       an authentic record under another valid key slot               (`key_specs`)
  length    an authentic record opened with len off by -1, +1, -16, +16    (`length_specs`)
"""
from __future__ import annotations

from dataclasses import dataclass, replace

import numpy as np

from oracle import oracle as O

OVERHEAD = 28  # tag 16 + nonce 12
ROOM = 16  # bytes every slot keeps past its record, so that an open with len + 16 reads inside the slot

BIT_LENGTHS = (0, 1, 15, 16, 17, 33)
LONG_LENGTHS = (1350, 4081, 9000)
RESIDUE_LENGTHS = tuple(16 * k + r for k in range(6) for r in range(16))
FIELD_LENGTHS = (1, 17, 33, 1350)
FIELDS = ("tag_zero", "tag_ones", "tag_other", "nonce_other", "ct_other")
KEY_LENGTHS = (0, 17, 33, 1350)
LENGTH_LENGTHS = (17, 33, 1350)
LENGTH_DELTAS = (-1, 1, -16, 16)


@dataclass(frozen=True)
class Spec:
    kind: str
    L: int  # payload length of the base record
    what: str  # the forgery in words, for failure messages
    bit: int = -1  # bit / bit_long / residue: the flipped bit, counted from Raw[0] (bit i of byte i // 8)
    field: str = ""  # field: one of FIELDS
    delta: int = 0  # length: what is added to the sealed length
    key: int = 0  # index into the batch's key list (the descriptor paths spread specs over keys)


def _bit(kind, L, bit):
    byte = bit >> 3
    part = "header" if byte < 4 else "ciphertext" if byte < 4 + L else "tag" if byte < 4 + L + 16 else "nonce"
    return Spec(kind, L, f"bit {bit & 7} of byte {byte} ({part})", bit=bit)


def bit_specs(L: int) -> list[Spec]:
    return [_bit("bit", L, b) for b in range(8 * (4 + L + OVERHEAD))]


def bit_long_specs(L: int, seed: int = 0) -> list[Spec]:
    rng = np.random.default_rng([0xB17, L, seed])
    nfull = L >> 4
    bits = list(range(32))  # the header
    bits += [8 * (4 + L) + b for b in range(128 + 96)]  # tag, then nonce
    # ciphertext edges: first block, last full block, partial block, and the blocks where the counter's
    # second byte changes (block 254 is counter 256)
    edges = {0, 15, 16, 16 * nfull - 1, 16 * nfull, L - 1} | {4063, 4064, 4079, 4080}
    for byte in sorted(e for e in edges if 0 <= e < L):
        bits.append(8 * (4 + byte) + int(rng.integers(8)))
    for blk in range((L + 15) >> 4):  # one bit somewhere in every block
        byte = 16 * blk + int(rng.integers(min(16, L - 16 * blk)))
        bits.append(8 * (4 + byte) + int(rng.integers(8)))
    return [_bit("bit_long", L, b) for b in bits]


def residue_specs() -> list[Spec]:
    # a different tag bit for every length; 37 is odd, so the 96 lengths visit all four tag words
    return [_bit("residue", L, 8 * (4 + L) + (37 * i + 5) % 128) for i, L in enumerate(RESIDUE_LENGTHS)]


def field_specs(lengths=FIELD_LENGTHS) -> list[Spec]:
    return [Spec("field", L, f, field=f) for L in lengths for f in FIELDS]


def key_specs(lengths=KEY_LENGTHS) -> list[Spec]:
    return [Spec("key", L, "descriptor names another valid key") for L in lengths for _ in range(2)]


def length_specs(lengths=LENGTH_LENGTHS) -> list[Spec]:
    return [Spec("length", L, f"sealed length {d:+d}", delta=d) for L in lengths for d in LENGTH_DELTAS]


def on_keys(specs, nkeys: int, first: int = 0) -> list[Spec]:
    """The specs dealt round-robin over key list entries first .. first + nkeys - 1."""
    return [replace(s, key=first + i % nkeys) for i, s in enumerate(specs)]


def uniform_groups(specs) -> dict[int, list[Spec]]:
    """The specs by payload length, for the uniform calls (one call per length)."""
    out: dict[int, list[Spec]] = {}
    for s in specs:
        out.setdefault(s.L, []).append(s)
    return out


@dataclass
class Batch:
    arena: np.ndarray  # uint8: every slot, forged ones included, gaps random
    offs: np.ndarray  # uint64
    lens: np.ndarray  # uint32: the length each packet is opened with (L + 28, or off by the `length` delta)
    kidx: np.ndarray  # uint32: key slot of each packet
    L: np.ndarray  # int64: payload length of the record in the slot
    size: np.ndarray  # int64: bytes of the slot, gap included
    kind: np.ndarray  # "auth" or the forgery kind
    specs: list  # specs[i]: the Spec of packet i, None for an authentic one
    keys: bytes  # the key table kidx indexes (32 bytes a slot)
    aad_len: int
    stride: int  # the uniform stride, 0 for packed slots

    @property
    def n(self) -> int:
        return len(self.offs)

    @property
    def forged(self) -> np.ndarray:
        return self.kind != "auth"

    def record(self, i: int, arena=None) -> np.ndarray:
        """The bytes packet i is opened on: data[4 : 4 + lens[i]] of its slot."""
        a = self.arena if arena is None else arena
        o = int(self.offs[i])
        return a[o + 4:o + 4 + int(self.lens[i])]

    def describe(self, i: int) -> str:
        s = self.specs[i]
        return (f"packet {i} at {int(self.offs[i])}: authentic, L={int(self.L[i])}" if s is None else
                f"packet {i} at {int(self.offs[i])}: {s.kind}, L={s.L}, {s.what}") + f", key {int(self.kidx[i])}"


def build(keys: bytes, key_slots, specs, seed: int, aad_len: int = 4, uniform: bool = False, align: int = 16,
          base: int = 0) -> Batch:
    """Slots 0, 2, .., 2F authentic, slot 2j + 1 forged by specs[j].

    keys: the key table (32 bytes a slot); key_slots: the valid slots in use -- spec.key indexes this list,
    and a `key` forgery names the list's next entry.  uniform: every slot has the same size (a multiple of
    `align`), else slots are packed at `align` with a random gap of 0..2 units each.  base: offset of slot 0
    (4 puts every record at 4 mod 16)."""
    assert specs and align % 4 == 0 and base % 4 == 0
    key_slots = [int(k) for k in key_slots]
    rng = np.random.default_rng([0xF026ED, seed, aad_len])
    F = len(specs)
    n = 2 * F + 1
    spec_of = [specs[min(i // 2, F - 1)] for i in range(n)]  # an authentic slot has its forged neighbour's shape
    L = np.array([s.L for s in spec_of], dtype=np.int64)
    kl = np.array([s.key for s in spec_of], dtype=np.int64)  # index into key_slots
    need = (4 + L + OVERHEAD + ROOM + align - 1) // align * align
    size = np.full(n, need.max()) if uniform else need + align * rng.integers(0, 3, n)
    offs = base + np.concatenate([[0], np.cumsum(size)[:-1]])
    arena = rng.integers(0, 256, base + int(size.sum()), dtype=np.uint8)  # headers, plaintexts and gaps
    kidx = np.array([key_slots[k] for k in kl], dtype=np.uint32)

    # the authentic packets, sealed in place; plaintexts, headers and nonces are all different
    auth = np.arange(0, n, 2)
    O.aesgo_seal_descs(keys, arena, offs[auth].astype(np.uint64), L[auth].astype(np.uint32), kidx[auth],
                       rng.integers(0, 256, 12 * len(auth), dtype=np.uint8), aad_len, 8)

    # per (key, length): the base record that is forged, and another authentic one for the splices
    pairs = sorted({(s.key, s.L) for s in specs})
    rec = {p: 4 + p[1] + OVERHEAD for p in pairs}
    side_offs = np.concatenate([[0], np.cumsum([2 * rec[p] for p in pairs])[:-1]]).astype(np.int64)
    side = rng.integers(0, 256, int(sum(2 * rec[p] for p in pairs)), dtype=np.uint8)
    so = np.array([o + j * rec[p] for p, o in zip(pairs, side_offs) for j in (0, 1)], dtype=np.uint64)
    O.aesgo_seal_descs(keys, side, so, np.array([p[1] for p in pairs for _ in (0, 1)], dtype=np.uint32),
                       np.array([key_slots[p[0]] for p in pairs for _ in (0, 1)], dtype=np.uint32),
                       rng.integers(0, 256, 12 * len(so), dtype=np.uint8), aad_len, 1)
    base_rec = {p: (side[o:o + rec[p]], side[o + rec[p]:o + 2 * rec[p]]) for p, o in zip(pairs, side_offs)}

    lens = (L + OVERHEAD).astype(np.uint32)
    kind = np.array(["auth"] * n, dtype=object)
    per_packet = [None] * n
    for j, s in enumerate(specs):
        i = 2 * j + 1
        b, other = base_rec[(s.key, s.L)]
        r = b.copy()
        tag, nonce = 4 + s.L, 4 + s.L + 16
        if s.kind in ("bit", "bit_long", "residue"):
            assert 0 <= s.bit < 8 * len(r)
            r[s.bit >> 3] ^= 1 << (s.bit & 7)
        elif s.kind == "field":
            if s.field == "tag_zero":
                r[tag:nonce] = 0
            elif s.field == "tag_ones":
                r[tag:nonce] = 0xFF
            elif s.field == "tag_other":
                r[tag:nonce] = other[tag:nonce]
            elif s.field == "nonce_other":
                r[nonce:] = other[nonce:]
            elif s.field == "ct_other":  # header and ciphertext of the other record, tag and nonce of this one
                r[:tag] = other[:tag]
            else:
                raise ValueError(s.field)
        elif s.kind == "key":
            assert len(key_slots) > 1
            kidx[i] = key_slots[(s.key + 1) % len(key_slots)]
        elif s.kind == "length":
            assert abs(s.delta) <= ROOM and s.L + s.delta >= 0
            lens[i] = s.L + OVERHEAD + s.delta
        else:
            raise ValueError(s.kind)
        o = int(offs[i])
        arena[o:o + len(r)] = r
        kind[i] = s.kind
        per_packet[i] = s
    return Batch(arena, offs.astype(np.uint64), lens, kidx, L, size.astype(np.int64), kind, per_packet, keys, aad_len,
                 int(size[0]) if uniform else 0)


def oracle_open(b: Batch, threads: int = 8):
    """What an open of the batch must leave: (status, arena) as O.aesgo_open_descs leaves them."""
    exp = b.arena.copy()
    status = np.full(b.n, 0x5A, dtype=np.uint8)
    O.aesgo_open_descs(b.keys, exp, b.offs, b.lens, b.kidx, status, b.aad_len, threads)
    return status, exp


def mismatches(b: Batch, status, arena, want_status, want_arena, limit: int = 6) -> str:
    """'' when status and arena equal the oracle's, else the first packets that differ, by index, kind,
    length and bit."""
    status, arena = np.asarray(status), np.asarray(arena)
    if np.array_equal(status, want_status) and np.array_equal(arena, want_arena):
        return ""
    out = []
    for i in range(b.n):
        o, z = int(b.offs[i]), int(b.size[i])
        st = int(status[i]) != int(want_status[i])
        diff = np.flatnonzero(arena[o:o + z] != want_arena[o:o + z])
        if st or len(diff):
            out.append(f"{b.describe(i)}: status {int(status[i])} (oracle {int(want_status[i])})" +
                       (f", {len(diff)} bytes differ from slot byte {int(diff[0])}" if len(diff) else ""))
            if len(out) == limit:
                break
    lead = int(b.offs[0])
    if not out and not np.array_equal(arena[:lead], want_arena[:lead]):
        out.append("bytes before the first slot differ")
    total = int((status != want_status).sum())
    return f"{total} statuses differ; first packets: " + "; ".join(out)


# ---------------- the matrices the tests use ----------------

def short_matrix() -> list[Spec]:
    """Every single-bit flip of the short records: 8 (32 + L) packets a length, 2192 in all."""
    return [s for L in BIT_LENGTHS for s in bit_specs(L)]


def full_matrix(with_descriptor_kinds: bool = True) -> list[Spec]:
    specs = short_matrix()
    for L in LONG_LENGTHS:
        specs += bit_long_specs(L)
    specs += residue_specs() + field_specs()
    if with_descriptor_kinds:
        specs += key_specs() + length_specs()
    return specs


# plain numbers, asserted by test_forgery_cases.py: a generator that silently makes fewer cases fails
COUNTS = {"bit": 2192, "bit_long": 1695, "residue": 96, "field": 20, "key": 8, "length": 12}


def header_flip_outside_aad(s: Spec | None, aad_len: int) -> bool:
    """A `bit` forgery on a header byte the additional data does not cover: the one forgery that opens."""
    return s is not None and s.kind in ("bit", "bit_long") and (s.bit >> 3) < 4 and (s.bit >> 3) >= aad_len
