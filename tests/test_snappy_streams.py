"""CPU: the host snappy decoders on every valid stream form and its near-misses (tests/snappy_streams.py).

The encoder tests never leave the encoder's image (shortest literal headers, copies of 4..64 bytes, no
4-byte offsets, the shortest preamble); a peer may send the rest.  Here the corpus built element by
element -- copies of every kind, offset and length at the limits of the output, literals in every header
form at every alignment, headers cut where zero bytes would complete them, every preamble length, random
valid streams -- goes through qgcm_snappy_uncompress and qgcm_snappy_uncompress_slots, and the result of
each stream (fails or not, and its bytes) must be oracle/snappy_oracle.py's, which in turn must give the
builder's own plaintext on every stream built as valid.  libsnappy 1.1.8, where present, must agree too."""
import ctypes as C
import os

import numpy as np
import pytest

import snappy_streams as SS
from quantum_amd import _lib

BIG = 16384 + 64  # above every total of a valid stream of the corpus


def slots_expectation(streams, wants, stride, cap, fill=0xA5):
    """The arena of `streams` (slot i: 4 bytes, then the stream, the rest `fill`) and what a slot decoder
    with output cap `cap` must leave: a decoded packet at [4, 4 + u), every other byte as it was; a stream
    that fails, or decodes to nothing, untouched with its length."""
    n = len(streams)
    host = np.full((n, stride), fill, dtype=np.uint8)
    lens = np.empty(n, np.uint32)
    for i, s in enumerate(streams):
        host[i, 4:4 + len(s)] = np.frombuffer(s, np.uint8)
        lens[i] = len(s)
    ref, rlens, rst = host.copy(), lens.copy(), np.zeros(n, np.uint8)
    for i, w in enumerate(wants):
        if w is not None and 0 < len(w) <= cap:
            ref[i, 4:4 + len(w)] = np.frombuffer(w, np.uint8)
            rlens[i] = len(w)
            rst[i] = 1
    return host, lens, ref, rlens, rst


def first_diff(a, b):
    """Index of the first differing element (for the assertion message), or None."""
    d = np.flatnonzero(np.asarray(a).reshape(-1) != np.asarray(b).reshape(-1))
    return None if d.size == 0 else int(d[0])


def test_corpus_self_check():
    corpus, wants = SS.corpus(), SS.oracle_results()
    valid = [s for s, w in zip(corpus, wants) if w is not None]
    assert len(corpus) > 50000
    assert 4 * len(valid) >= len(corpus) and 4 * (len(corpus) - len(valid)) >= len(corpus)
    feats = set().union(*(s.feats for s in valid))
    need = {("copy", k) for k in (1, 2, 3)} | {("lit", f) for f in range(5)}
    need |= {("ip", r) for r in range(4)} | {("op", r) for r in range(4)}
    assert need <= feats, need - feats
    assert len(set(s.data for s in corpus)) > 0.95 * len(corpus)  # few repeats
    assert SS.CHAIN_TOTAL <= max(len(w) for w in wants if w is not None) < BIG


def test_oracle_equals_builder_plaintext():
    built_valid = 0
    for s, w in zip(SS.corpus(), SS.oracle_results()):
        if s.plain is not None:
            built_valid += 1
            assert w == s.plain, s.data[:64].hex()
        else:
            assert w is None, s.data[:64].hex()  # built to be invalid: the oracle says so too
    assert built_valid > 20000


def test_host_uncompress_equals_oracle():
    L = _lib.lib()
    dst = C.create_string_buffer(BIG + 8)
    guard = b"\x5a" * 8

    def run(data, cap):
        C.memmove(C.addressof(dst) + cap, guard, 8)
        n = L.qgcm_snappy_uncompress(data, len(data), dst, cap)
        assert C.string_at(C.addressof(dst) + cap, 8) == guard  # nothing past the cap
        return None if n < 0 else C.string_at(dst, n)

    for s, w in zip(SS.corpus(), SS.oracle_results()):
        assert run(s.data, BIG) == w, s.data[:64].hex()
        want_len = L.qgcm_snappy_uncompressed_length(s.data, len(s.data))
        if w is not None:
            assert want_len == len(w)
            # the cap at the byte: the total fits exactly, and not into one byte less
            assert run(s.data, len(w)) == w
            if w:
                assert run(s.data, len(w) - 1) is None


def test_host_uncompress_slots_equals_oracle():
    L = _lib.lib()
    corpus, wants = SS.corpus(), SS.oracle_results()
    big_stride = (4 + L.qgcm_snappy_max_compressed_length(SS.CHAIN_TOTAL) + 3) // 4 * 4
    small = [i for i, s in enumerate(corpus) if len(s.data) <= 2108]
    large = [i for i, s in enumerate(corpus) if len(s.data) > 2108] + small[::64]
    for idx, stride in ((small, 2112), (large, big_stride)):
        assert idx and max(len(corpus[i].data) for i in idx) <= stride - 4
        host, lens, ref, rlens, rst = slots_expectation([corpus[i].data for i in idx], [wants[i] for i in idx],
                                                        stride, stride - 4)
        assert 0 < int(rst.sum()) < len(idx)
        got = host.copy()
        st = np.full(len(idx), 7, np.uint8)
        bad = L.qgcm_snappy_uncompress_slots(got.ctypes.data, stride, len(idx), lens.ctypes.data, st.ctypes.data, 4)
        assert bad == int((rst == 0).sum())
        assert np.array_equal(st, rst), first_diff(st, rst)
        assert np.array_equal(lens, rlens), first_diff(lens, rlens)
        d = first_diff(got, ref)
        assert d is None, (d // stride, d % stride)
    # an empty result is dropped: b"\x00" is in the corpus, valid for the codec, and its slot stays
    i = [k for k, s in enumerate(corpus) if s.data == b"\x00"][0]
    assert wants[i] == b"" and i in small


def test_libsnappy_equals_oracle():
    path = "/opt/conda/lib/libsnappy.so.1"
    if not os.path.exists(path):
        pytest.skip("libsnappy not present")
    lib = C.CDLL(path)
    lib.snappy_uncompress.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.POINTER(C.c_size_t)]
    out = C.create_string_buffer(BIG)
    for s, w in zip(SS.corpus(), SS.oracle_results()):
        n = C.c_size_t(BIG)
        rc = lib.snappy_uncompress(s.data, len(s.data), out, C.byref(n))
        got = C.string_at(out, n.value) if rc == 0 else None
        assert got == w, s.data[:64].hex()
