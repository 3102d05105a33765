"""GPU: the device snappy codec on every valid stream form, and in every LDS layout run_snappy chooses.

Decoders (snappy_uncompress_kernel, snappy_uncompress_group_kernel): the corpus of
tests/snappy_streams.py -- what a peer may send and the project's encoder never emits: copies of every kind
and length at the limits of the output, literals in every header form at every alignment, headers cut
where the staging's zeroed slack would complete them, every preamble, random valid streams.  Bar: status,
length and every byte of the arena equal to oracle/snappy_oracle.py's result laid into the slot (a failed or
empty-result slot and its length untouched, every byte outside the output unchanged).

Encoders (snappy_compress_kernel, snappy_compress_group_kernel): max_len across the three layouts (four
packets per wave within 64 KiB of LDS a workgroup, over 64 KiB, one wave per packet), every hash-table
size.  Bar: the whole arena and the lengths equal to the host encoder's (pinned to libsnappy's bytes by
tests/test_snappy.py), failures restored whole, and the device decoder restores every packet."""
import numpy as np
import pytest

import snappy_inputs as SI
import snappy_streams as SS
from oracle import snappy_oracle
from test_gpu_snappy import _host_compress, _lib, _run, encoder, encoder_ctxs, torch  # noqa: F401  (fixtures)
from test_snappy_streams import first_diff, slots_expectation

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def refs():
    """References computed once and shared by both codec settings; dropped with the module."""
    cache = {}
    yield cache
    cache.clear()


def _cached(refs, key, make):
    if key not in refs:
        refs[key] = make()
    return refs[key]


def _expect_decode(host, lens, wants, cap):
    """What a slot decoder with output cap `cap` leaves of the arena `host`."""
    ref, rlens, rst = host.copy(), lens.copy(), np.zeros(len(wants), np.uint8)
    for i, w in enumerate(wants):
        if w is not None and 0 < len(w) <= cap:
            ref[i, 4:4 + len(w)] = np.frombuffer(w, np.uint8)
            rlens[i] = len(w)
            rst[i] = 1
    return ref, rlens, rst


def _decode_and_check(torch, ctx, refs, key, streams, wants, stride, max_len, cap):
    """One snappy_uncompress call over `streams` (one a slot, the arena pre-filled with 0xA5): status,
    lengths and the whole arena against the expectation."""
    assert max(len(s) for s in streams) <= max_len <= stride - 4 and cap <= stride - 4
    host, lens = _cached(refs, (key, stride), lambda: slots_expectation(streams, wants, stride, 0)[:2])
    ref, rlens, rst = _cached(refs, (key, stride, cap), lambda: _expect_decode(host, lens, wants, cap))
    arena = torch.from_numpy(host.reshape(-1)).cuda()
    dlens = torch.from_numpy(lens.view(np.int32)).cuda()
    out, ol, st = _run(torch, ctx, False, arena, stride, len(streams), dlens, max_len, cap)
    assert np.array_equal(st, rst), (first_diff(st, rst), streams[first_diff(st, rst)][:48].hex())
    assert np.array_equal(ol, rlens), first_diff(ol, rlens)
    d = first_diff(out, ref)
    assert d is None, (d // stride, d % stride, streams[d // stride][:48].hex())
    return rst


def _pick(idx, seed):
    """The corpus streams `idx` and their oracle results, shuffled: valid and invalid, short and long
    streams neighbour each other, so the four groups of a wave diverge."""
    corpus, wants = SS.corpus(), SS.oracle_results()
    order = np.random.default_rng(seed).permutation(np.unique(np.asarray(idx)))
    return [corpus[i].data for i in order], [wants[i] for i in order]


# The layouts (run_snappy): the group decoder's region per packet is
#   a16(max_len + 24) + a16(cap + 8) + 64 bytes, four a wave, and it runs while 4 * region <= 65536.
# stride 2112: max_len = cap = 2108 -> 4 * (2144 + 2128 + 64) = 17344: the group decoder.
# stride 8160, cap 8152 (a16(8160) = 8160):
#   max_len 8136: a16(8160) = 8160 -> 4 * (8160 + 8160 + 64) = 65536: the last group layout;
#   max_len 8137: a16(8161) = 8176 -> 4 * (8176 + 8160 + 64) = 65600: the first wave layout;
#   and from the other side, max_len 8136 with cap 8153: a16(8161) = 8176 -> 65600, the wave layout.
# stride 19152 = 4 + max_compressed_length(16384) rounded up: max_len 19146, cap 16384, far past the step.
SMALL = 2108


def _layout(name):
    corpus, wants = SS.corpus(), SS.oracle_results()
    small = [i for i, s in enumerate(corpus) if len(s.data) <= SMALL]
    # the long streams, and the short ones with long outputs (they fail by the cap in the small slots)
    large = [i for i, s in enumerate(corpus) if len(s.data) > SMALL or (wants[i] is not None and len(wants[i]) > SMALL)]
    if name == "small":
        return _pick(small, 0x5EED0081)
    if name == "step":
        return _pick(large + small[::16], 0x5EED0082)
    return _pick(large + small[::32], 0x5EED0083)


@pytest.mark.parametrize("cap", [2108, 2000])
def test_decoder_corpus_group_layout(torch, encoder, refs, cap):
    """Every stream of up to 2108 bytes in 2112-byte slots, four packets a wave (one a wave under
    wave_codec).  cap 2108 is the largest total the slots hold (the corpus has totals of 2107..2116 on both
    sides of it); cap 2000 puts more streams over the cap (totals of 1999..2001 are in the corpus)."""
    streams, wants = _cached(refs, "small", lambda: _layout("small"))
    rst = _decode_and_check(torch, encoder, refs, "small", streams, wants, 2112, SMALL, cap)
    over = sum(1 for w in wants if w is not None and len(w) > cap)
    assert over > 50 and 20000 < int(rst.sum()) < len(streams) - 20000
    assert {len(w) for w in wants if w is not None} >= {cap - 1, cap, cap + 1}


@pytest.mark.parametrize("max_len,cap", [(8136, 8152), (8137, 8152), (8136, 8153)])
def test_decoder_corpus_at_the_group_to_wave_step(torch, encoder, refs, max_len, cap):
    """The longest streams (offsets of 4095, literals of 4096) and a sixteenth of the rest, just below and
    just above the step from the group layout to the wave layout (the arithmetic is above)."""
    streams, wants = _cached(refs, "step", lambda: _layout("step"))
    a16 = lambda x: (x + 15) & ~15  # noqa: E731
    assert (4 * (a16(max_len + 24) + a16(cap + 8) + 64) <= 65536) == ((max_len, cap) == (8136, 8152))
    rst = _decode_and_check(torch, encoder, refs, "step", streams, wants, 8160, max_len, cap)
    assert 1000 < int(rst.sum()) < len(streams) - 1000
    assert {len(w) for w in wants if w is not None} >= {8152, 8153}


@pytest.mark.parametrize("cap", [16384, 16383])
def test_decoder_corpus_wave_layout_16k(torch, encoder, refs, cap):
    """The device's longest streams and outputs: the chains of overlapping 64-byte copies that fill 16384
    bytes, with the long streams and a thirty-second of the rest.  cap 16384 is the largest total the
    device takes (the 16385-byte stream fails); under cap 16383 the full chains fail too."""
    in_max = _lib().qgcm_snappy_max_compressed_length(16384)  # the decoder's input limit
    stride = (4 + in_max + 3) // 4 * 4
    streams, wants = _cached(refs, "16k", lambda: _layout("16k"))
    rst = _decode_and_check(torch, encoder, refs, "16k", streams, wants, stride, in_max, cap)
    chains = [i for i, w in enumerate(wants) if w is not None and len(w) == SS.CHAIN_TOTAL]
    assert len(chains) >= len(SS.CHAIN_OFFS) + 1 and all(rst[i] == (cap == 16384) for i in chains)
    assert any(w is not None and len(w) == 16385 for w in wants)


@pytest.mark.parametrize("stride", [64, 1472, 1700])
def test_decoder_prefetch_cover(torch, encoder, refs, stride):
    """The group codecs prefetch the first 1.5 KiB of a slot, less where the slot is shorter: strides 64 and
    1472 are below that cover, 1700 above it, with streams on both sides of 1536 bytes.  The random valid
    streams and a slice of the copy corpus, whichever fit the slot."""

    def make():
        corpus = SS.corpus()
        idx = list(SS.section("random_streams")) + list(SS.section("copies"))[::7]
        idx = [i for i in idx if len(corpus[i].data) <= stride - 4]
        streams, want = _pick(idx, 0x5EED0084 + stride)
        if stride > 1540:  # single literals: streams of 1525..1566 bytes, and the longest the slot holds
            for n in list(range(1520, 1560)) + [stride - 4 - 7]:
                for form in (2, 3, 4):
                    s = SS.build([SS.L(SS.fill(n, n), form)])
                    assert len(s.data) <= stride - 4 and snappy_oracle.decode(s.data) == s.plain
                    at = (7 * n + form) % len(streams)
                    streams.insert(at, s.data)
                    want.insert(at, s.plain)
        return streams, want

    streams, wants = _cached(refs, ("cover", stride), make)
    rst = _decode_and_check(torch, encoder, refs, ("cover", stride), streams, wants, stride, stride - 4, stride - 4)
    assert int(rst.sum()) > (100 if stride == 64 else 3000)
    if stride > 1540:
        assert sum(1 for s, ok in zip(streams, rst) if ok and len(s) > 1536) > 50


# ---------------------------------------------------------------------------------------------
# encoders

ENC_KINDS = SI.KINDS + ["ab", "acgt"]
ENC_LENS = [0, 1, 16, 17, 18] + [(1 << p) + d for p in range(8, 15) for d in (-1, 0, 1)]


def _packet(kind, n, seed):
    if kind in ("ab", "acgt"):  # two- and four-letter alphabets: hash collisions, long matches at short offsets
        rng = np.random.default_rng(0x5EED0090 + 131 * seed + n)
        return bytes(rng.choice(np.frombuffer(kind.encode(), np.uint8), n))
    return SI.make(kind, n, seed=seed)


def _enc_stride(max_len):
    return (4 + _lib().qgcm_snappy_max_compressed_length(max_len) + 3) // 4 * 4


def _enc_pool(max_len):
    """Packets of every kind at every length of ENC_LENS up to max_len, and one of max_len + 1; each three
    times in a shuffled batch (over a thousand packets: more than one round of the kernels' grid-stride
    loops, so the next packets' prefetch runs), with the host encoder's stream of each."""
    base = [_packet(k, n, seed) for seed in range(2 if max_len < 4096 else 1) for k in ENC_KINDS
            for n in ENC_LENS if n <= max_len]
    base.append(_packet("half", max_len + 1, 9))
    comps = [_host_compress(p) for p in base]
    reps = -(-1100 // len(base))
    order = np.random.default_rng(0x5EED0091 + max_len).permutation(np.repeat(np.arange(len(base)), reps))
    return [base[i] for i in order], [comps[i] for i in order]


def _enc_arena(payloads, stride, seed):
    """Slots pre-filled with random bytes (a pattern, so that a restore from the wrong offset shows)."""
    n = len(payloads)
    host = np.random.default_rng(seed).integers(0, 256, (n, stride), dtype=np.uint8)
    for i, p in enumerate(payloads):
        host[i, 4:4 + len(p)] = np.frombuffer(p, np.uint8)
    return host, np.array([len(p) for p in payloads], np.uint32)


def _expect_compress(host, payloads, comps, max_len, limit):
    """The host encoder's arena: a packet over max_len, or whose stream is over `limit`, stays whole."""
    ref, rlens, rst = host.copy(), np.array([len(p) for p in payloads], np.uint32), np.zeros(len(payloads), np.uint8)
    for i, (p, c) in enumerate(zip(payloads, comps)):
        if len(p) <= max_len and len(c) <= limit:
            ref[i, 4:4 + len(c)] = np.frombuffer(c, np.uint8)
            rlens[i] = len(c)
            rst[i] = 1
    return ref, rlens, rst


def _compress_and_check(torch, ctx, host, lens, payloads, comps, stride, max_len, limit):
    ref, rlens, rst = _expect_compress(host, payloads, comps, max_len, limit)
    arena = torch.from_numpy(host.reshape(-1)).cuda()
    dlens = torch.from_numpy(lens.view(np.int32)).cuda()
    out, ol, st = _run(torch, ctx, True, arena, stride, len(payloads), dlens, max_len, limit)
    assert np.array_equal(st, rst), (first_diff(st, rst), limit)
    assert np.array_equal(ol, rlens), (first_diff(ol, rlens), limit)
    d = first_diff(out, ref)
    assert d is None, (d // stride, d % stride, len(payloads[d // stride]), limit)
    return out, ol, rst


@pytest.mark.parametrize("max_len", [1468, 2048, 4096, 4097, 6000, 8192, 8193, 12000, 16384])
def test_encoder_across_layouts(torch, encoder, refs, max_len):
    """limit = max_len: four packets a wave up to max_len 8192 (4 * (table + a16(max_len + 24)) bytes of LDS
    a workgroup: 22400 at 1468, 49280 at 4096, 82048 at 4097 -- over 64 KiB -- and 98432 at 8192), one wave
    a packet from 8193 on; hash tables of 2^8 .. 2^14 entries by the packet's length in each.  The slot is
    just large enough for max_compressed_length(max_len).  Device arena and lengths equal to the host
    encoder's, tails and failed packets (max_len + 1 bytes; a stream over the limit) untouched; then the
    device decoder restores every packet."""
    stride = _enc_stride(max_len)
    payloads, comps = _cached(refs, ("pool", max_len), lambda: _enc_pool(max_len))
    host, lens = _cached(refs, ("enc_arena", max_len), lambda: _enc_arena(payloads, stride, 0x5EED0092 + max_len))
    out, ol, rst = _compress_and_check(torch, encoder, host, lens, payloads, comps, stride, max_len, max_len)
    assert 0 < int((rst == 0).sum()) < len(payloads) // 4
    # and back: a failed slot still holds its packet, which the decoder takes for a stream (the oracle says
    # what becomes of it)
    wants = [p if ok else snappy_oracle.decode(p) for p, ok in zip(payloads, rst)]
    ref, rlens, rst2 = _expect_decode(out, ol, wants, max_len)
    back, bl, st2 = _run(torch, encoder, False, torch.from_numpy(out.reshape(-1).copy()).cuda(), stride, len(payloads),
                         torch.from_numpy(ol.view(np.int32).copy()).cuda(),
                         _lib().qgcm_snappy_max_compressed_length(max_len), max_len)
    assert np.array_equal(st2, rst2), first_diff(st2, rst2)
    assert np.array_equal(bl, rlens), first_diff(bl, rlens)
    d = first_diff(back, ref)
    assert d is None, (d // stride, d % stride)


@pytest.mark.parametrize("max_len", [1468, 8192, 16384], ids=["group_64k", "group_over_64k", "wave"])
def test_encoder_limit_at_the_byte(torch, encoder, refs, max_len):
    """A compressible and an incompressible packet among others, in each layout: limit == the stream's
    length succeeds, one less fails with the slot restored whole; the incompressible packet also with
    len < limit < stream length (its overflow is written past the packet's own bytes, which come back too);
    limit == 0 fails every packet."""
    stride = _enc_stride(max_len)

    def make():
        pool, pool_c = _cached(refs, ("pool", max_len), lambda: _enc_pool(max_len))
        payloads, comps = list(pool[:61]), list(pool_c[:61])
        n = max_len - 100
        for at, p in ((13, _packet("words", n, 3)), (30, _packet("random", n, 4)), (31, _packet("line", n, 5))):
            payloads.insert(at, p)
            comps.insert(at, _host_compress(p))
        return payloads, comps, _enc_arena(payloads, stride, 0x5EED0093 + max_len)

    payloads, comps, (host, lens) = _cached(refs, ("limits", max_len), make)
    n = max_len - 100
    c_words, c_random = len(comps[13]), len(comps[30])
    assert c_words < n < n + 1 < c_random <= stride - 4
    for limit in (c_words, c_words - 1, c_random, c_random - 1, n + 1, n, 0):
        _, _, rst = _compress_and_check(torch, encoder, host, lens, payloads, comps, stride, max_len, limit)
        assert rst[13] == (limit >= c_words) and rst[30] == (limit >= c_random)
        assert (limit == 0) == (not rst.any())
