"""The seal matrix (seal_cases.py) is sound, on the CPU: the counts are asserted in plain numbers, so a
generator that silently makes fewer cases fails here; the layouts visit every slot offset mod 16 against
every L mod 16 and every L mod 64 with both nonce forms; and for every batch the GPU tests seal, OpenSSL
leaves the same arena as the restated oracle, the seal touches nothing but payload, tag and nonce, and the
oracle's open of the result accepts every packet and gives the plaintext back."""
import numpy as np
import pytest

import seal_cases as SC
from oracle import oracle as O


def test_counts():
    assert len(SC.SEAL_LENGTHS) == SC.COUNTS["lengths"] and len(SC.DESC_LENGTHS) == SC.COUNTS["desc_lengths"]
    assert len(set(SC.SEAL_LENGTHS)) == len(SC.SEAL_LENGTHS) and max(SC.DESC_LENGTHS) == 9000
    assert set(range(131)) <= set(SC.SEAL_LENGTHS)
    assert {16 * k + j for k in range(9, 68) for j in (0, 1)} <= set(SC.SEAL_LENGTHS)
    for L in (2015, 2016, 2017, 2031, 2032, 2033, 2047, 2048, 2049, 1349, 1350, 1351, 1353, 1433, 4047, 4048, 4049, 4063,
              4064, 4065, 4079, 4080, 4081, 4095, 4096, 4097, 8191, 8192, 8193, 8159, 8160, 8161, 9000, 32719, 32720, 32721):
        assert L in SC.SEAL_LENGTHS, L
    # every block count up to 68, every count of GHASH exponents (d + 2) up to 70
    assert {(L + 15) >> 4 for L in SC.SEAL_LENGTHS} >= set(range(69))
    for config in SC.QUAD_CONFIGS:
        assert sum(SC.quad_case(L, config).n for L in SC.SEAL_LENGTHS) == SC.COUNTS["quad_packets"]
    one = [L for L in SC.SEAL_LENGTHS if L <= SC.ONE_CAP_LEN]
    assert sum(SC.one_case(L, "s16", True).n for L in one) == SC.COUNTS["one_packets"]
    assert SC.per_wave_case(True).n == SC.COUNTS["per_wave"] and SC.segmented_case(False).n == SC.COUNTS["segmented"]
    assert SC.descs_one_case(True).n == SC.COUNTS["descs_one"]
    assert len(SC.PER_PACKET_LENGTHS) == SC.COUNTS["per_packet"]
    assert sum(1 for _ in SC.all_batches()) == 4 * 285 + 3 * 131 + 4 * 284 + 7 + 2 * 4


def test_quad_layouts_cover_offsets_residues_and_nonce_forms():
    seen, by_form = set(), {False: set(), True: set()}
    partial_owner_j0 = set()
    for config, (lead, stride, from_slot) in SC.QUAD_CONFIGS.items():
        for L in SC.SEAL_LENGTHS:
            b = SC.quad_case(L, config)
            assert (b.nonces is None) == from_slot and b.lead == lead and b.stride == SC.STRIDES[stride](L)
            seen |= {(int(o) % 16, L % 16) for o in b.offs}
            by_form[from_slot].add(L % 64)
            partial_owner_j0.add(((L >> 4) & 3, ((L + 15) >> 4) & 3, L & 15))
    assert seen == {(o, r) for o in (0, 4, 8, 12) for r in range(16)}
    assert by_form[False] == by_form[True] == set(range(64))
    # nfull & 3 (owner of the partial block) x d & 3 (the lane with E_K(J0)) x L & 15: every combination there is
    assert partial_owner_j0 == {(nf, (nf + (1 if r else 0)) & 3, r) for nf in range(4) for r in range(16)}
    # the minimal stride is minimal, leaves no room, and the last slot ends where the trail begins
    b = SC.quad_case(17, "min4_array")
    assert b.stride == 52 and b.end == b.n * 52 and len(b.arena) == b.end + SC.TRAIL
    # one configuration at least walks a length through all four offsets with the nonce in the slot
    assert {int(o) % 16 for o in SC.quad_case(17, "min4_slot").offs} == {0, 4, 8, 12}


def test_descriptor_layouts():
    b = SC.per_wave_case(False)
    assert sorted(b.lens.tolist()) == list(SC.DESC_LENGTHS) and len(set(b.kidx.tolist())) == 5
    assert (b.offs % 4 == 0).all() and {int(o) % 16 for o in b.offs} == {0, 4, 8, 12} and b.lead == 4
    gaps = b.size - ((4 + b.lens.astype(np.int64) + SC.OVERHEAD + 3) & ~3)
    assert set(gaps.tolist()) == {0, 4, 8}
    s = SC.segmented_case(True)
    per_key = np.bincount(s.kidx)
    assert per_key[8] == SC.SEG_MIN_PACKETS and (np.delete(per_key, 8) < SC.SEG_MIN_PACKETS).all()
    assert (per_key > 0).sum() == 17 and set(s.lens[s.kidx == 8].tolist()) == set(SC.DESC_LENGTHS)
    assert sorted(s.lens[s.kidx != 8].tolist()) == list(range(131))
    d = SC.descs_one_case(True)
    assert (d.offs % 16 == 0).all() and (d.size % 16 == 0).all() and d.nonces is None


def _check(name, b):
    status, want = SC.oracle_seal(b)
    assert status.tolist() == [1] * b.n
    # independent code: OpenSSL leaves the same arena
    assert np.array_equal(SC.openssl_seal(b), want), f"{name}: OpenSSL and the oracle disagree: " + \
        SC.mismatches(b, None, SC.openssl_seal(b), status, want)
    # nothing but [4, 4 + L + 28) of each slot changes (the nonce too when it was in the slot already)
    keep = np.ones(len(b.arena), bool)
    span = 4 + b.lens.astype(np.int64) + SC.OVERHEAD
    for o, z in zip(b.offs.astype(np.int64).tolist(), span.tolist()):
        keep[o + 4:o + z] = False
    assert np.array_equal(want[keep], b.arena[keep]), name
    nonce_at = (b.offs.astype(np.int64) + span - 12)[:, None] + np.arange(12)
    nonces = b.slot_nonces() if b.nonces is None else b.nonces
    assert np.array_equal(want[nonce_at].reshape(-1), nonces), name
    # the oracle's open accepts every record and restores the plaintext
    back = want.copy()
    st = np.full(b.n, 0x5A, np.uint8)
    O.aesgo_open_descs(b.keys, back, b.offs, (b.lens + SC.OVERHEAD).astype(np.uint32), b.kidx, st, b.aad_len, 8)
    assert st.tolist() == [1] * b.n, name
    pay = keep.copy()
    for o, L in zip(b.offs.astype(np.int64).tolist(), b.lens.tolist()):
        pay[o + 4:o + 4 + L] = True
    assert np.array_equal(back[pay], b.arena[pay]), name
    if b.n > 1 and int(b.lens[0]) > 0:  # the packets differ from each other
        assert not np.array_equal(want[int(b.offs[0]) + 4:int(b.offs[0]) + 20], want[int(b.offs[1]) + 4:int(b.offs[1]) + 20])


@pytest.mark.parametrize("part", range(4))
def test_oracle_and_openssl_agree_on_every_batch(part):
    """Every batch the GPU tests seal, a quarter of them a case."""
    for k, (name, b) in enumerate(SC.all_batches()):
        if k % 4 == part:
            _check(name, b)


def test_mismatches_names_the_byte():
    b = SC.quad_case(18, "min4_slot")
    status, want = SC.oracle_seal(b)
    assert SC.mismatches(b, status, want, status, want) == ""
    got = want.copy()
    o = int(b.offs[3])
    got[o + 4 + 18 + 28] ^= 0xFF  # the first gap byte of packet 3
    msg = SC.mismatches(b, status, got, status, want)
    assert "packet 3 at" in msg and f"({o % 16} mod 16)" in msg and "L=18" in msg and "slot byte 50 (gap)" in msg
    st = status.copy()
    st[2] = 0
    assert "packet 2" in SC.mismatches(b, st, want, status, want)
    got = want.copy()
    got[0] ^= 1
    assert "before the first slot" in SC.mismatches(b, status, got, status, want)
    got = want.copy()
    got[-1] ^= 1
    assert "behind the last slot" in SC.mismatches(b, status, got, status, want)
