"""The forged-record generator (forgery_cases.py) is sound: on the CPU, the oracle accepts every packet it
labels authentic and rejects every forged one -- except a flipped header byte the additional data does
not cover, which it accepts -- leaves a rejected packet with a zeroed plaintext and everything else
untouched, and OpenSSL gives the same verdict on every packet.  The per-kind counts are asserted in plain
numbers, so a generator that silently makes fewer cases fails here."""
import numpy as np
import pytest

import forgery_cases as FC
from oracle import oracle as O

NKEYS = 5


@pytest.fixture(scope="module")
def keys():
    return np.random.default_rng(0xF0C5).bytes(32 * NKEYS)


def _ossl_verdict(b, i):
    """OpenSSL's verdict on packet i as crypto/aes.go:57-62 cuts it: nonce = the last 12 bytes, tag = the
    16 before them."""
    r = bytes(b.record(i))
    L = len(r) - FC.OVERHEAD
    o = int(b.offs[i])
    aad = bytes(b.arena[o:o + b.aad_len])
    k = int(b.kidx[i])
    return O.ossl_gcm_open(b.keys[32 * k:32 * k + 32], r[L + 16:], aad, r[:L], r[L:L + 16])


def _check(b):
    before = b.arena
    status, after = FC.oracle_open(b)
    assert set(np.unique(status)) <= {0, 1}
    for i in range(b.n):
        s = b.specs[i]
        o, z, lo = int(b.offs[i]), int(b.size[i]), int(b.lens[i]) - FC.OVERHEAD
        want = 1 if s is None or FC.header_flip_outside_aad(s, b.aad_len) else 0
        assert status[i] == want, b.describe(i)
        pt = _ossl_verdict(b, i)
        assert (pt is not None) == bool(want), "OpenSSL disagrees: " + b.describe(i)
        slot, was = after[o:o + z], before[o:o + z]
        assert np.array_equal(slot[:4], was[:4]) and np.array_equal(slot[4 + lo:], was[4 + lo:]), b.describe(i)
        if want:
            assert bytes(slot[4:4 + lo]) == pt, b.describe(i)
        else:
            assert not slot[4:4 + lo].any(), b.describe(i)
    assert np.array_equal(after[:int(b.offs[0])], before[:int(b.offs[0])])
    # neighbours of a forged packet are authentic and differ from each other
    f = np.flatnonzero(b.forged)
    assert np.array_equal(f, np.arange(1, b.n, 2))
    for i in f[:: max(1, len(f) // 64)]:
        lo, hi = int(b.offs[i - 1]), int(b.offs[i + 1])
        n = min(4 + int(b.L[i - 1]), 4 + int(b.L[i + 1])) + 16  # header, payload, tag
        assert not np.array_equal(after[lo:lo + n], after[hi:hi + n])


def test_full_matrix_counts_and_verdicts(keys):
    specs = FC.on_keys(FC.full_matrix(), NKEYS)
    counts = {k: sum(s.kind == k for s in specs) for k in FC.COUNTS}
    assert counts == {"bit": 2192, "bit_long": 1695, "residue": 96, "field": 20, "key": 8, "length": 12}
    assert counts == FC.COUNTS and len(specs) == 4023
    for L in FC.BIT_LENGTHS:  # every bit of the record, once
        bits = sorted(s.bit for s in specs if s.kind == "bit" and s.L == L)
        assert bits == list(range(8 * (32 + L)))
    assert {L: sum(s.kind == "bit_long" and s.L == L for s in specs) for L in FC.LONG_LENGTHS} == \
        {1350: 347, 4081: 519, 9000: 829}
    for L in FC.LONG_LENGTHS:
        bits = {s.bit for s in specs if s.kind == "bit_long" and s.L == L}
        assert set(range(32)) <= bits and set(range(8 * (4 + L), 8 * (4 + L + 28))) <= bits
        blocks = {((b >> 3) - 4) >> 4 for b in bits if 4 <= (b >> 3) < 4 + L}
        assert blocks == set(range((L + 15) >> 4))
    res = [s for s in specs if s.kind == "residue"]
    assert {(s.L & 15, (s.L >> 4) & 3) for s in res} == {(r, q) for r in range(16) for q in range(4)}
    assert {((s.bit >> 3) - 4 - s.L) >> 2 for s in res} == {0, 1, 2, 3}  # every tag word
    assert all(4 + s.L <= (s.bit >> 3) < 4 + s.L + 16 for s in res)
    b = FC.build(keys, range(NKEYS), specs, seed=1, base=4)
    assert b.n == 2 * 4023 + 1 and all(int(o) % 16 == 4 for o in b.offs)
    _check(b)


@pytest.mark.parametrize("aad_len", [0, 1, 3])
def test_short_matrix_short_additional_data(keys, aad_len):
    specs = FC.short_matrix()
    b = FC.build(keys, [2], specs, seed=2, aad_len=aad_len)
    accepted = sum(FC.header_flip_outside_aad(s, aad_len) for s in specs)
    assert accepted == len(FC.BIT_LENGTHS) * 8 * (4 - aad_len)
    _check(b)


def test_uniform_form_has_one_stride(keys):
    for L, group in FC.uniform_groups(FC.short_matrix() + FC.residue_specs()).items():
        b = FC.build(keys, [1], group, seed=3, uniform=True, align=64)
        assert b.stride % 64 == 0 and b.stride >= 4 + L + 28 + FC.ROOM
        assert np.array_equal(b.offs, np.arange(b.n, dtype=np.uint64) * b.stride)
        assert (b.lens == L + 28).all() and len(b.arena) == b.n * b.stride
    _check(b)
