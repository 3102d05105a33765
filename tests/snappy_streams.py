"""A builder of snappy block streams from element lists, and the stream corpora the CPU and GPU decoder
tests share (tests/test_snappy_streams.py, tests/test_gpu_snappy_streams.py).

The project's encoder (golang/snappy's block encoder) emits a small part of the format: literals in
their shortest header form, copies of 4..64 bytes, no 4-byte-offset copy, no literal header with 3 or 4
length bytes, the shortest preamble.  A peer may send every other form, so the decoders are fed streams
built here, element by element, in every form the format allows -- and the near-misses of each form.

The builder states the format on its own (format_description.txt of google/snappy): it runs no decoder.
build() returns, with the stream's bytes, the plaintext its elements describe, or None where the stream
was built to be invalid.  Pure Python, no GPU, no library; every corpus is deterministic."""
from __future__ import annotations

import functools
import random
from typing import NamedTuple


class Stream(NamedTuple):
    data: bytes
    plain: bytes | None  # what the elements describe; None for a stream built to be invalid
    feats: frozenset     # ("lit", form), ("copy", kind), ("ip", header position & 3), ("op", output position & 3)


def uvarint(n: int, pad: int = 0) -> bytes:
    """The shortest little-endian base-128 form of n, then `pad` overlong continuation bytes (the last
    byte gets its continuation bit, a zero group follows)."""
    out = bytearray()
    while n >= 0x80:
        out.append((n & 0x7F) | 0x80)
        n >>= 7
    out.append(n)
    for _ in range(pad):
        out[-1] |= 0x80
        out.append(0)
    return bytes(out)


def lit_forms(length: int) -> list[int]:
    """The header forms that can express a literal of `length` bytes."""
    return [f for f in range(5) if (length <= 60 if f == 0 else length <= 256 ** f)]


def literal_header(length: int, form: int) -> bytes:
    n = length - 1
    if form == 0:
        assert 0 <= n < 60
        return bytes([n << 2])
    assert 1 <= form <= 4 and 0 <= n < 256 ** form
    return bytes([(59 + form) << 2]) + n.to_bytes(form, "little")


def literal(data: bytes, form: int) -> bytes:
    """Form 0: the length in the tag; forms 1..4: tags 60..63 with that many length bytes (any length the
    form can express, canonical or not)."""
    return literal_header(len(data), form) + bytes(data)


def copy_kinds(off: int, ln: int) -> list[int]:
    """The copy kinds that can express (off, ln)."""
    kinds = []
    if 4 <= ln <= 11 and off < 2048:
        kinds.append(1)
    if 1 <= ln <= 64:
        if off < 65536:
            kinds.append(2)
        kinds.append(3)
    return kinds


def copy(kind: int, off: int, ln: int) -> bytes:
    """Kind 1: len 4..11, off < 2048 (2 bytes); kinds 2 and 3: len 1..64, a 2- or 4-byte offset."""
    if kind == 1:
        assert 4 <= ln <= 11 and 0 <= off < 2048
        return bytes([(off >> 8) << 5 | (ln - 4) << 2 | 1, off & 0xFF])
    assert 1 <= ln <= 64
    if kind == 2:
        assert 0 <= off < 65536
        return bytes([(ln - 1) << 2 | 2]) + off.to_bytes(2, "little")
    assert kind == 3 and 0 <= off < 1 << 32
    return bytes([(ln - 1) << 2 | 3]) + off.to_bytes(4, "little")


def L(data: bytes, form: int | None = None):
    """A literal element; form None = the shortest that fits."""
    return ("lit", bytes(data), lit_forms(len(data))[0] if form is None else form)


def K(kind: int, off: int, ln: int):
    """A copy element."""
    return ("copy", kind, off, ln)


def build(elements, total: int | None = None, pad: int = 0) -> Stream:
    """The stream of `elements` behind the preamble uvarint(total, pad); total defaults to the length of
    the plaintext the elements describe.  plain is None where the format calls the stream invalid: a
    preamble over five bytes, a copy with offset 0 or from before the output, output past `total` at any
    element, or an output that does not end at `total`."""
    out, ok = _plain_of(elements, total)
    head = uvarint(len(out) if total is None else total, pad)
    data = bytearray(head)
    feats = set()
    op = 0
    for e in elements:
        feats.add(("ip", len(data) & 3))
        feats.add(("op", op & 3))
        if e[0] == "lit":
            feats.add(("lit", e[2]))
            data += literal(e[1], e[2])
            op += len(e[1])
        else:
            feats.add(("copy", e[1]))
            data += copy(e[1], e[2], e[3])
            op += e[3]
    if len(head) > 5 or (total is not None and total != len(out)):
        ok = False
    return Stream(bytes(data), bytes(out) if ok else None, frozenset(feats))


def _plain_of(elements, total: int | None = None):
    """(plaintext, well-formed) of an element list: literals append their bytes, a copy appends `ln` bytes
    one at a time from `off` back (so that it may overlap what it writes)."""
    out, ok = bytearray(), True
    for e in elements:
        if e[0] == "lit":
            out += e[1]
        else:
            _, _, off, ln = e
            if off == 0 or off > len(out):
                ok = False
                out += bytes(ln)
            else:
                for _ in range(ln):
                    out.append(out[-off])
        if total is not None and len(out) > total:
            ok = False
    return out, ok


def invalid(data: bytes) -> Stream:
    """Raw bytes built to be invalid (a cut stream, a hand-made preamble)."""
    return Stream(bytes(data), None, frozenset())


def fill(n: int, seed: int) -> bytes:
    return random.Random(0x5EED0000 + seed).randbytes(n)


def _ones(k: int, seed: int):
    """k one-byte literals: they move the next header to another ip & 3 and its output to another op & 3."""
    return [L(bytes([0x41 + (seed + j) % 26]), 0) for j in range(k)]


# ---------------------------------------------------------------------------------------------
# (a) copies

A_OFFS = list(range(1, 71)) + [255, 256, 257, 2047, 2048, 2049, 4095]
CHAIN_OFFS = (1, 2, 3, 5, 63, 64, 65)
CHAIN_TOTAL = 16384


def copies() -> list[Stream]:
    """Every (off, len, kind) at op == off and op == off + 3, each with three near-misses: `total` one
    smaller (the copy overruns by a byte), off == op + 1, off == 0.  Then a copy as the first element, and
    chains of overlapping 64-byte copies that fill 16384 bytes."""
    out = []
    for off in A_OFFS:
        for lead in (off, off + 3):
            pre = L(fill(lead, 131 * off + lead))
            for ln in range(1, 65):
                for kind in copy_kinds(off, ln):
                    els = [pre, K(kind, off, ln)]
                    out.append(build(els))
                    out.append(build(els, total=lead + ln - 1))
                    if kind in copy_kinds(lead + 1, ln):
                        out.append(build([pre, K(kind, lead + 1, ln)]))
                    out.append(build([pre, K(kind, 0, ln)]))
    for kind, ln in ((1, 4), (2, 1), (2, 64), (3, 1), (3, 64)):  # a copy at op == 0
        for off in (0, 1, 4):
            out.append(build([K(kind, off, ln)]))
            out.append(build([K(kind, off, ln), L(b"tail")]))
    for off in CHAIN_OFFS + (0,):  # 0: the offsets in turn
        offs = CHAIN_OFFS if off == 0 else (off,)
        els = [L(fill(64, 7000 + off), j % 2 + 1) for j in range(2)]  # 128 bytes, then 254 copies of 64
        for j in range((CHAIN_TOTAL - 128) // 64):
            els.append(K(2 + j % 2, offs[j % len(offs)], 64))
        out.append(build(els))
        out.append(build(els, total=CHAIN_TOTAL - 1))
        out.append(build(els[:-1] + [K(2, offs[0], 63)]))  # ends one byte short of the chains' total ...
        out.append(build(els[:-1] + [K(2, offs[0], 63)], total=CHAIN_TOTAL))  # ... and says it does not
    return out


# ---------------------------------------------------------------------------------------------
# (b) literals

B_LENS = list(range(1, 71)) + [255, 256, 257, 1024, 4096]


def literals() -> list[Stream]:
    """Every length in every header form that can express it, behind 0..3 one-byte literals (the header at
    every ip & 3, the payload at every op & 3); each cut by 1..5 bytes, with a declared length one more than
    the bytes present, and with a length one more than total - op."""
    out = []
    for n in B_LENS:
        data = fill(n, 9000 + n)
        for form in lit_forms(n):
            for lead in range(4):
                els = _ones(lead, n) + [L(data, form)]
                good = build(els)
                out.append(good)
                for cut in range(1, 6):
                    out.append(invalid(good.data[:-cut]))
                if form in lit_forms(n + 1):  # the header says n + 1, n bytes follow
                    head = build(_ones(lead, n), total=lead + n + 1).data
                    out.append(invalid(head + literal_header(n + 1, form) + data))
                out.append(build(els, total=lead + n - 1))
    return out


# ---------------------------------------------------------------------------------------------
# (c) headers that end at, or past, the end of the input

def cut_headers() -> list[Stream]:
    """Streams cut inside their last element's header, where the missing bytes, read as zero, would give a
    valid element (a decoder that reads its zeroed slack past the input without a bounds check accepts
    them): a copy-2 with off < 256 cut after its low offset byte, a copy-4 with off < 256 cut by 1..4
    bytes, literal tags 60..63 of one zero byte cut inside their length bytes and payload.  Then every prefix
    of one stream with all four tag kinds."""
    out = []
    for lead in range(4):
        for off in (1, 2, 5, 60, 255):
            pre = _ones(lead, off) + [L(fill(off, 300 + off))]
            for ln in (1, 4, 11, 64):
                good = build(pre + [K(2, off, ln)])
                out += [good, invalid(good.data[:-1])]
                good = build(pre + [K(3, off, ln)])
                out.append(good)
                out += [invalid(good.data[:-cut]) for cut in (1, 2, 3, 4)]
        for form in (1, 2, 3, 4):
            for pre in (_ones(lead, form), _ones(lead, form) + [L(fill(9, form))]):
                good = build(pre + [L(b"\x00", form)])  # tag, `form` zero length bytes, a zero payload byte
                out.append(good)
                out += [invalid(good.data[:-cut]) for cut in range(1, form + 2)]
    els = [L(b"snappy!"), K(1, 7, 9), L(fill(13, 77), 1), K(2, 20, 33), L(b"xyz", 2), K(3, 5, 2), L(b"end", 4)]
    whole = build(els)
    assert 40 <= len(whole.data) <= 60
    out.append(whole)
    out += [invalid(whole.data[:k]) for k in range(len(whole.data))]
    return out


# ---------------------------------------------------------------------------------------------
# (d) preamble

CAPS = (60, 1468, 2000, 2108, 8152, 16384)  # the output caps the tests run with: totals at and one over each


def compact(total: int, seed: int = 0) -> list:
    """A short element list of `total` output bytes: a literal of up to 60 bytes, then 64-byte copies."""
    first = min(total, 60)
    els, n = [L(fill(first, 500 + total + seed))], first
    while n < total:
        ln = min(64, total - n)
        els.append(K(2 + (n >> 6) % 2, 1 + (n * 7 + seed) % min(n, 60), ln))
        n += ln
    return els


def preambles() -> list[Stream]:
    """Preambles of 1..5 bytes, overlong ones included, and of six; a fifth byte of 0x0f and of 0x10; totals
    at and one over each cap in CAPS; an output one short of `total`; one element too many; the empty
    stream and b"\\x00"."""
    out = []
    for total in (1, 5, 127, 128, 300, 16383, 16384):
        els = compact(total)
        for pad in range(0, 7 - len(uvarint(total))):  # up to six bytes: the last is invalid
            out.append(build(els, pad=pad))
    body = literal(b"hello", 0)
    for head in (b"\x85\x80\x80\x80\x00", b"\x85\x80\x80\x80\x0f", b"\x85\x80\x80\x80\x10", b"\x85\x80\x80\x80\x80\x00",
                 b"\x85\x80\x80\x80\x80", b"\xff\xff\xff\xff\x0f", b"\xff\xff\xff\xff\x10", b"\x85\x80\x80\x80\x8f",
                 b"\x85\x80\x80\x80", b"\x85\x80", b"\x85"):
        ok = head == b"\x85\x80\x80\x80\x00"
        out.append(Stream(head + body, b"hello" if ok else None, frozenset()))
        out.append(invalid(head))
    for cap in CAPS:
        for total in (cap - 1, cap, cap + 1):
            out.append(build(compact(total, 1)))
            out.append(build(compact(total, 2), total=total + 1))  # the output one short of total
            out.append(build(compact(total, 3) + [L(b"x")], total=total))  # one element too many
            out.append(build(compact(total, 4) + [K(2, 1, 1)], total=total))
    out += [invalid(b""), Stream(b"\x00", b"", frozenset()), invalid(b"\x00\x00"), invalid(b"\x00\x01\x00")]
    return out


# ---------------------------------------------------------------------------------------------
# (e) valid random streams

E_MAX = 1468  # a 1472-B slot's packet: the longest output, and the longest stream, of this corpus


def random_streams(count: int = 3000, seed: int = 0x5EED0E) -> list[Stream]:
    """Random element lists drawn from every literal form and copy kind, with now and then an overlong
    preamble: outputs, and streams, of up to E_MAX bytes, all valid."""
    rng = random.Random(seed)
    out = []
    while len(out) < count:
        target = rng.choice((rng.randint(1, 64), rng.randint(1, 400), rng.randint(1, E_MAX), E_MAX))
        pad = rng.choice((0, 0, 0, 1, 2))
        els, n, size = [], 0, 5
        while n < target:
            room = target - n
            if n == 0 or rng.random() < 0.4:
                ln = min(room, rng.choice((1, 2, 3, rng.randint(1, 70), rng.randint(1, 300))))
                e = L(rng.randbytes(ln), rng.choice(lit_forms(ln)))
                cost = 1 + e[2] + ln
            else:
                off = min(n, rng.choice((1, 2, 3, rng.randint(1, 70), rng.randint(1, n), n)))
                ln = min(room, rng.choice((1, 2, 3, rng.randint(1, 64), 64)))
                kind = rng.choice(copy_kinds(off, ln))
                e = K(kind, off, ln)
                cost = (2, 3, 5)[kind - 1]
            if size + cost > E_MAX:
                break
            els.append(e)
            size += cost
            n += len(e[1]) if e[0] == "lit" else e[3]
        s = build(els, pad=pad)
        assert s.plain is not None and len(s.data) <= E_MAX and len(s.plain) <= E_MAX
        out.append(s)
    return out


@functools.lru_cache(maxsize=None)
def _parts():
    return tuple((f.__name__, tuple(f())) for f in (copies, literals, cut_headers, preambles, random_streams))


@functools.lru_cache(maxsize=None)
def corpus() -> tuple[Stream, ...]:
    """(a)-(e), built once per process."""
    return tuple(s for _, part in _parts() for s in part)


def section(name: str) -> range:
    """The indices in corpus() of one corpus: "copies", "literals", "cut_headers", "preambles",
    "random_streams"."""
    at = 0
    for part, streams in _parts():
        if part == name:
            return range(at, at + len(streams))
        at += len(streams)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def oracle_results() -> tuple:
    """oracle.snappy_oracle.decode of every stream of corpus(): the expected result of every test (the
    builder itself runs no decoder).  Computed once per process and left unchanged."""
    from oracle import snappy_oracle

    return tuple(snappy_oracle.decode(s.data) for s in corpus())
