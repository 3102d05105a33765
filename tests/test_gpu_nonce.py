"""GPU: nonces drawn on the device from each context's AES-256-CTR generator (include/qgcm.h
qgcm_nonce_fill / qgcm_nonce_seed / QGCM_NONCES_GENERATE; quantum_amd/csrc/nonce_rng.h).

Nonce j of a seeded stream is the first 12 bytes of AES-256_K(BE128(V0 + j)); the oracle's block cipher
says what that is, and the oracle's seal says what a packet sealed with it looks like.  Every test makes
its own context(s), so a seeded generator never reaches the session `ctx` fixture.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

AAD = bytes([10, 99, 0, 1])
# SP 800-38A F.5.5 (CTR-AES256.Encrypt): key, initial counter, and the first output block's first 12 bytes
F55_KEY = bytes.fromhex("603deb1015ca71be2b73aef0857d77811f352c073b6108d72d9810a30914dff4")
F55_CTR = bytes.fromhex("f0f1f2f3f4f5f6f7f8f9fafbfcfdfeff")
F55_FIRST = "0bdf7df1591716335e9a8b15"
GEN_KEY = bytes((0x3C + 11 * i) & 0xFF for i in range(32))  # a generator key that is no packet key
MAX_PAYLOAD = 1 << 28  # QGCM_MAX_PAYLOAD


@pytest.fixture(scope="module")
def torch():
    import torch as T

    if not T.cuda.is_available():
        pytest.skip("no GPU")
    return T


@pytest.fixture
def make_ctx(torch):
    """Fresh contexts, closed after the test."""
    from quantum_amd.crypto import Context

    made = []

    def make(max_keys=4):
        c = Context(device=0, max_keys=max_keys)
        made.append(c)
        return c

    yield make
    for c in made:
        c.close()


_STREAMS = {}


def stream(key: bytes, v0: int, count: int, first: int = 0) -> np.ndarray:
    """Positions [first, first + count) of the stream seeded with (key, v0): a (count, 12) uint8 array from
    the oracle's AES-256 (computed once per seed and grown on demand)."""
    have = _STREAMS.get((key, v0))
    if have is None or len(have) < first + count:
        rk = O.aes256_expand(key)
        out = C.create_string_buffer(16)
        rows = [] if have is None else [have]
        for j in range(0 if have is None else len(have), first + count):
            O.lib().oracle_aes256_encrypt_block(rk, ((v0 + j) % (1 << 128)).to_bytes(16, "big"), out)
            rows.append(np.frombuffer(out.raw[:12], np.uint8).reshape(1, 12))
        have = np.concatenate(rows)
        have.setflags(write=False)
        _STREAMS[(key, v0)] = have
    return have[first:first + count]


def seed(ctx, key: bytes, v0: int) -> None:
    from quantum_amd import batch

    batch.nonce_seed(ctx, key, (v0 % (1 << 128)).to_bytes(16, "big"))


def fill(torch, ctx, n: int, stream_=None):
    from quantum_amd import batch

    out = torch.zeros(12 * n, dtype=torch.uint8, device="cuda")
    batch.nonce_fill(ctx, out, n, stream=stream_)
    return out


def distinct(nonces: np.ndarray) -> bool:
    rows = np.ascontiguousarray(nonces.reshape(-1, 12))
    return len(np.unique(rows.view([("", rows.dtype)] * 12))) == len(rows)


def host_buffer(nbytes: int, pinned: bool):
    from quantum_amd import _lib

    if pinned:
        ptr = _lib.lib().qgcm_host_alloc(nbytes)
        assert ptr
        arr = np.frombuffer((C.c_uint8 * nbytes).from_address(ptr), dtype=np.uint8)
        return arr, ptr, lambda: _lib.lib().qgcm_host_free(ptr)
    arr = np.zeros(nbytes, dtype=np.uint8)
    return arr, arr.ctypes.data, lambda: None


def slot_nonces(arena: np.ndarray, offs, lens) -> np.ndarray:
    at = (np.asarray(offs, np.int64) + 4 + np.asarray(lens, np.int64) + 16)[:, None] + np.arange(12)
    return np.ascontiguousarray(arena[at])


# ---- 1. known answer ----

def test_known_answer_sp800_38a_f55(torch, make_ctx):
    ctx = make_ctx()
    seed(ctx, F55_KEY, int.from_bytes(F55_CTR, "big"))
    got = fill(torch, ctx, 4).cpu().numpy().reshape(4, 12)
    want = np.stack([np.frombuffer(O.aes256_encrypt_block(
        F55_KEY, ((int.from_bytes(F55_CTR, "big") + j) % (1 << 128)).to_bytes(16, "big"))[:12], np.uint8) for j in range(4)])
    # the publication's first keystream block is ciphertext block 1 xor plaintext block 1 of F.5.5
    pub = bytes(a ^ b for a, b in zip(bytes.fromhex("601ec313775789a5b7a7f504bbf3d228"),
                                      bytes.fromhex("6bc1bee22e409f96e93d7e117393172a")))
    assert O.aes256_encrypt_block(F55_KEY, F55_CTR) == pub and pub[:12].hex() == F55_FIRST
    assert np.array_equal(got, want), (got[0].tobytes().hex(), want[0].tobytes().hex())
    assert got[0].tobytes().hex() == F55_FIRST


# ---- 2. stream identity across the carries ----

@pytest.mark.parametrize("v0", [(1 << 32) - 3, (1 << 64) - 3, (1 << 128) - 3], ids=["carry32", "carry64", "wrap128"])
def test_stream_identity(torch, make_ctx, v0):
    """Every nonce of a fill equals the oracle's, the counter carrying out of 32 and 64 bits and wrapping at
    2^128; the output sits 4 bytes past a 16-byte boundary between two 64-byte guards that stay as they were."""
    from quantum_amd import batch

    ctx = make_ctx()
    for n in (1, 63, 64, 65, 257, 4099):
        seed(ctx, GEN_KEY, v0)
        buf = torch.full((16 + 4 + 64 + 12 * n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        base = (-buf.data_ptr()) % 16 + 4 + 64  # out = 16-byte boundary + 4, after a guard of 64 bytes
        out = buf[base:base + 12 * n]
        assert out.data_ptr() % 16 == 4
        batch.nonce_fill(ctx, out, n)
        host = buf.cpu().numpy()
        assert np.array_equal(host[base:base + 12 * n].reshape(n, 12), stream(GEN_KEY, v0, n)), n
        assert (host[:base] == 0xA5).all() and (host[base + 12 * n:] == 0xA5).all(), n


# ---- 3. continuation, and two streams at once ----

def test_continuation_and_two_streams(torch, make_ctx):
    ctx = make_ctx()
    v0 = 0x0123456789ABCDEF << 40
    seed(ctx, GEN_KEY, v0)
    a, b = fill(torch, ctx, 5), fill(torch, ctx, 7)
    got = torch.cat([a, b]).cpu().numpy().reshape(12, 12)
    assert np.array_equal(got, stream(GEN_KEY, v0, 12))
    # two fills of 1000 on two streams, neither synchronized before both are issued
    seed(ctx, GEN_KEY, v0)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    o1 = fill(torch, ctx, 1000, s1)
    o2 = fill(torch, ctx, 1000, s2)
    s1.synchronize()
    s2.synchronize()
    h1, h2 = o1.cpu().numpy().reshape(1000, 12), o2.cpu().numpy().reshape(1000, 12)
    want = stream(GEN_KEY, v0, 2000)
    assert np.array_equal(h1, want[:1000]) and np.array_equal(h2, want[1000:])  # reserved in call order
    assert distinct(np.concatenate([h1, h2]))


# ---- 4. uniform batches ----

def uniform_arena(rng, n, L, stride):
    host = rng.integers(0, 256, n * stride, dtype=np.uint8)
    host.reshape(n, stride)[:, :4] = np.frombuffer(AAD, np.uint8)
    return host


@pytest.mark.parametrize("n,L,stride", [(1, 0, 32), (17, 1, 36), (17, 33, 68), (64, 1350, 1408), (2049, 15, 48),
                                        (2049, 16, 52)])
def test_seal_uniform_generate(torch, make_ctx, n, L, stride):
    """Both uniform paths: one workgroup per packet (n <= 2048, stride a multiple of 16) and the quad kernel.
    Slot j carries stream position j, the sealed bytes are the oracle's with that nonce, nothing between the
    nonce and the next slot changes, and the batch opens back."""
    from quantum_amd import batch

    ctx = make_ctx()
    key = bytes(range(64, 96))
    ctx.set_key(0, key)
    v0 = (1 << 64) - 9
    seed(ctx, GEN_KEY, v0)
    rng = np.random.default_rng(0x90CE + n + L)
    plain = uniform_arena(rng, n, L, stride)
    arena = torch.from_numpy(plain.copy()).cuda()
    status = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    before = ctx.launch_counts()
    batch.seal_uniform(ctx, arena, stride, n, L, 0, batch.GENERATE, status=status)
    after = ctx.launch_counts()
    want_kernel = "one" if n <= 2048 and stride % 16 == 0 else "quad"
    assert after[want_kernel] - before[want_kernel] == 1
    got = arena.cpu().numpy()
    want_nonces = stream(GEN_KEY, v0, n)
    assert np.array_equal(got.reshape(n, stride)[:, 4 + L + 16:4 + L + 28], want_nonces)
    ref = plain.copy()
    nn = np.ascontiguousarray(want_nonces).reshape(-1)
    O.lib().oracle_seal_uniform(key, ref.ctypes.data, stride, n, L, 4, nn.ctypes.data)
    assert np.array_equal(got, ref)  # ct || tag || nonce per slot, and every byte from 4+L+28 to the stride
    assert status.cpu().tolist() == [1] * n
    status.fill_(7)
    batch.open_uniform(ctx, arena, stride, n, L + 28, 0, status=status)
    assert status.cpu().tolist() == [1] * n
    back = arena.cpu().numpy().reshape(n, stride)
    assert np.array_equal(back[:, :4 + L], plain.reshape(n, stride)[:, :4 + L])


def test_seal_uniform_generate_refusals_draw_nothing(torch, make_ctx):
    """QGCM_E_KEY (unset key), QGCM_E_ARG (stride too small) and n = 0 leave the arena as it was and the
    generator where it was: the next good call starts at position 0 of the seeded stream."""
    from quantum_amd import _lib, batch

    ctx = make_ctx()
    key = bytes(range(32))
    ctx.set_key(0, key)
    v0 = 77
    seed(ctx, GEN_KEY, v0)
    n, L, stride = 40, 100, 144
    rng = np.random.default_rng(0x90CF)
    plain = uniform_arena(rng, n, L, stride)
    arena = torch.from_numpy(plain.copy()).cuda()
    Lb = _lib.lib()
    gen = _lib.NONCES_GENERATE
    assert Lb.qgcm_seal_uniform(ctx.handle, arena.data_ptr(), stride, n, L, 1, gen, 4, None, None) == _lib.QGCM_E_KEY
    assert Lb.qgcm_seal_uniform(ctx.handle, arena.data_ptr(), 64, n, L, 0, gen, 4, None, None) == _lib.QGCM_E_ARG
    assert Lb.qgcm_seal_uniform(ctx.handle, arena.data_ptr(), stride, 0, L, 0, gen, 4, None, None) == _lib.QGCM_OK
    assert Lb.qgcm_nonce_fill(ctx.handle, arena.data_ptr(), 0, None) == _lib.QGCM_OK
    assert Lb.qgcm_nonce_fill(ctx.handle, arena.data_ptr() + 1, 4, None) == _lib.QGCM_E_ARG
    torch.cuda.synchronize()
    assert np.array_equal(arena.cpu().numpy(), plain)
    batch.seal_uniform(ctx, arena, stride, n, L, 0, batch.GENERATE)
    got = arena.cpu().numpy().reshape(n, stride)
    assert np.array_equal(got[:, 4 + L + 16:4 + L + 28], stream(GEN_KEY, v0, n))


# ---- 5. descriptor batches ----

@pytest.mark.parametrize("desc_chunk", [None, "64"], ids=["one_launch", "desc_chunk_64"])
def test_seal_batch_generate(torch, make_ctx, desc_chunk, monkeypatch):
    """300 packets, slot offsets 4 mod 16, three key slots of which one is unset, one descriptor with a key
    index out of range and one with len = QGCM_MAX_PAYLOAD: the rejected ones keep every byte of their slots
    (the 12 nonce bytes too) and their stream positions; every other packet is the oracle's seal with the
    nonce at stream position = its batch index, also when the batch is cut into sorted chunks of 64
    (QGCM_DESC_CHUNK)."""
    from quantum_amd import batch

    if desc_chunk:
        monkeypatch.setenv("QGCM_DESC_CHUNK", desc_chunk)
    max_keys = 3
    ctx = make_ctx(max_keys)
    rng = np.random.default_rng(0x90D0)
    keys = rng.integers(0, 256, 32 * max_keys, dtype=np.uint8).tobytes()
    ctx.set_key(0, keys[:32])
    ctx.set_key(1, keys[32:64])  # slot 2 stays unset
    n = 300
    lens = rng.integers(0, 1501, n).astype(np.uint32)
    lens[:5] = [0, 1, 15, 16, 17]
    kidx = rng.integers(0, 3, n).astype(np.uint32)
    kidx[:5] = [0, 1, 0, 1, 0]
    out_of_range, too_long = 41, 137
    kidx[out_of_range] = max_keys + 5
    room = lens.astype(np.uint64).copy()  # the slot a descriptor owns (the too-long one owns a short slot)
    lens[too_long] = MAX_PAYLOAD
    kidx[too_long] = 0
    rec = ((4 + room + 28 + 15) & ~np.uint64(15))
    offs = (np.concatenate([[0], np.cumsum(rec)[:-1]]) + 4).astype(np.uint64)
    assert bool((offs % 16 == 4).all())
    size = int(offs[-1] + rec[-1]) + 64
    plain = rng.integers(0, 256, size, dtype=np.uint8)
    plain[offs.astype(np.int64)[:, None] + np.arange(4)] = np.frombuffer(AAD, np.uint8)
    v0 = (1 << 32) - 100
    seed(ctx, GEN_KEY, v0)
    arena = torch.from_numpy(plain.copy()).cuda()
    status = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    descs = batch.make_descs(offs, lens, kidx, "cuda")
    batch.seal_batch(ctx, arena, descs, n, batch.GENERATE, status=status)
    got = arena.cpu().numpy()
    ok = (kidx < 2) & (lens < MAX_PAYLOAD)
    assert not ok[out_of_range] and not ok[too_long] and int((kidx == 2).sum()) > 20
    assert np.array_equal(status.cpu().numpy(), ok.astype(np.uint8))
    vi = np.flatnonzero(ok)
    ref = plain.copy()
    O.aesgo_seal_descs(keys, ref, np.ascontiguousarray(offs[vi]), np.ascontiguousarray(lens[vi]),
                       np.ascontiguousarray(kidx[vi]), np.ascontiguousarray(stream(GEN_KEY, v0, n)[vi]).reshape(-1), 4)
    assert np.array_equal(got, ref)  # rejected slots and every gap byte-identical, the rest the oracle's
    assert np.array_equal(slot_nonces(got, offs[vi], lens[vi]), stream(GEN_KEY, v0, n)[vi])
    olens = np.where(ok, lens + 28, 28).astype(np.uint32)
    batch.open_batch(ctx, arena, batch.make_descs(offs, olens, kidx, "cuda"), n, status=status)
    assert np.array_equal(status.cpu().numpy()[vi], np.ones(len(vi), np.uint8))
    back = arena.cpu().numpy()
    for i in vi[::7]:
        o, L = int(offs[i]), int(lens[i])
        assert np.array_equal(back[o:o + 4 + L], plain[o:o + 4 + L]), i


# ---- 6. host batches ----

@pytest.mark.parametrize("n,mode", [(64, "direct"), (300, "direct"), (64, "pinned_copies"), (300, "pinned_copies"),
                                    (64, "pageable"), (300, "pageable"), (1500, "chunked")])
def test_seal_host_generate(torch, make_ctx, n, mode, monkeypatch):
    """qgcm_seal_host(..., GENERATE), L = 1350 in 1392-byte slots: a pinned arena sealed in place over PCIe
    (the nonces written over PCIe by the same kernel), the same arena with QGCM_HOST_DIRECT=0 (copies), a
    pageable arena, and a batch cut into three pipeline chunks (QGCM_PIPE_CHUNK_MB=1: one reservation, each
    chunk its part).  Every packet is the oracle's seal with the nonce found in its slot; the nonces are
    distinct and, the generator being seeded, packet j's is stream position j."""
    from quantum_amd import batch

    if mode == "pinned_copies":
        monkeypatch.setenv("QGCM_HOST_DIRECT", "0")
    if mode == "chunked":
        monkeypatch.setenv("QGCM_HOST_DIRECT", "0")
        monkeypatch.setenv("QGCM_PIPE_CHUNK_MB", "1")
    ctx = make_ctx()
    key = bytes(range(100, 132))
    ctx.set_key(0, key)
    L, stride = 1350, 1392
    v0 = (1 << 128) - 40
    seed(ctx, GEN_KEY, v0)
    rng = np.random.default_rng(0x90D1 + n)
    arena, aptr, free = host_buffer(n * stride, mode != "pageable")
    try:
        arena[:] = uniform_arena(rng, n, L, stride)
        plain = arena.copy()
        status = np.full(n, 7, np.uint8)
        before = ctx.launch_counts()
        assert batch.seal_host(ctx, aptr, stride, n, L, 0, batch.GENERATE, status_ptr=status.ctypes.data) == 0
        after = ctx.launch_counts()
        if mode == "chunked":
            assert after["quad"] - before["quad"] + after["one"] - before["one"] == 3  # 704 + 704 + 92 packets
        assert status.tolist() == [1] * n
        got = arena.copy()
        found = np.ascontiguousarray(got.reshape(n, stride)[:, 4 + L + 16:4 + L + 28])
        ref = plain.copy()
        O.lib().oracle_seal_uniform(key, ref.ctypes.data, stride, n, L, 4, found.reshape(-1).ctypes.data)
        assert np.array_equal(got, ref)
        assert distinct(found)
        assert np.array_equal(found, stream(GEN_KEY, v0, n))
    finally:
        del arena
        free()


# ---- 7. groups ----

@pytest.mark.parametrize("path", ["copy", "zerocopy", "dma", "direct"])
def test_group_seal_host_generate(torch, path, monkeypatch):
    """Two members on device 0, each path of qgcm_group_last_path (0 host copies: a pageable arena; 1 zero-copy:
    4-byte-packed records interleaved in a pinned arena; 2 DMA runs: the batch in qgcm_group_order's order; 3
    direct: 16-byte-aligned records in a pinned arena).  Each member draws from its own context's generator:
    seeded differently, member m's k-th packet carries position k of member m's stream.  All status 1, all
    nonces distinct, every packet the oracle's seal with its slot's nonce, and the batch opens back."""
    from quantum_amd import _lib, shard

    if path in ("copy", "zerocopy"):
        monkeypatch.setenv("QGCM_GROUP_DMA", "0")
    G, n, nkeys = 2, 1200, 24
    grp = shard.Group([0] * G, max_keys=64)
    try:
        rng = np.random.default_rng(0x90D2)
        keys = rng.integers(0, 256, 32 * nkeys, dtype=np.uint8).tobytes()
        grp.set_keys(0, keys)
        kidx = rng.integers(0, nkeys, n).astype(np.uint32)
        if path == "dma":
            kidx = kidx[grp.order(kidx)[0]]
        owner = shard.key_shard(kidx, G)
        assert len(set(owner.tolist())) == G
        lens = rng.integers(0, 1501, n).astype(np.uint32)
        align = 16 if path == "direct" else 4
        step = (4 + lens.astype(np.uint64) + 28 + align - 1) // align * align
        offs = np.concatenate([[0], np.cumsum(step)[:-1]]).astype(np.uint64)
        size = int(offs[-1] + step[-1]) + 16
        arena, aptr, free = host_buffer(size, path != "copy")
        try:
            arena[:] = rng.integers(0, 256, size, dtype=np.uint8)
            arena[offs.astype(np.int64)[:, None] + np.arange(4)] = np.frombuffer(AAD, np.uint8)
            plain = arena.copy()
            gen_keys = [bytes((0x51 + 3 * i + 97 * m) & 0xFF for i in range(32)) for m in range(G)]
            v0s = [(1 << 64) - 5, (1 << 96) + 12345]
            for m in range(G):
                seed(grp.member(m), gen_keys[m], v0s[m])
            status = np.full(n, 7, np.uint8)
            assert grp.seal_host(aptr, shard.host_descs(offs, lens, kidx), n, _lib.NONCES_GENERATE, 4,
                                 status.ctypes.data) == 0
            assert [grp.last_path(m) for m in range(G)] == [path] * G
            assert status.tolist() == [1] * n
            got = arena.copy()
            found = slot_nonces(got, offs, lens)
            ref = plain.copy()
            O.aesgo_seal_descs(keys, ref, offs, lens, kidx, found.reshape(-1), 4, 8)
            assert np.array_equal(got, ref)
            assert distinct(found)
            for m in range(G):
                mine = np.flatnonzero(owner == m)
                assert np.array_equal(found[mine], stream(gen_keys[m], v0s[m], len(mine))), m
            status[:] = 7
            assert grp.open_host(aptr, shard.host_descs(offs, lens + 28, kidx), n, 4, status.ctypes.data) == 0
            assert [grp.last_path(m) for m in range(G)] == [path] * G
            assert status.tolist() == [1] * n
            want = ref.copy()  # opened: plaintext back, tag || nonce left as sealed
            pay = np.zeros(size, bool)
            for o, L in zip(offs.astype(np.int64), lens.astype(np.int64)):
                pay[o + 4:o + 4 + L] = True
            want[pay] = plain[pay]
            assert np.array_equal(arena, want)
        finally:
            del arena
            free()
    finally:
        grp.close()


# ---- 8. production seeding and the reseed rule ----

def test_unseeded_contexts_never_collide(torch, make_ctx):
    a, b = make_ctx(), make_ctx()
    na, nb = fill(torch, a, 4096).cpu().numpy(), fill(torch, b, 4096).cpu().numpy()
    assert distinct(np.concatenate([na, nb]))


def test_reseed_interval(torch, make_ctx, monkeypatch):
    """QGCM_NONCE_RESEED=64 and an explicit seed: positions 0..63 are the seeded stream; the next call would
    take the count past the interval, so the generator takes a new key and counter from getrandom first --
    the next 64 do not continue the stream; all 128 are distinct."""
    monkeypatch.setenv("QGCM_NONCE_RESEED", "64")
    ctx = make_ctx()
    v0 = 5
    seed(ctx, GEN_KEY, v0)
    first = fill(torch, ctx, 64).cpu().numpy().reshape(64, 12)
    second = fill(torch, ctx, 64).cpu().numpy().reshape(64, 12)
    want = stream(GEN_KEY, v0, 128)
    assert np.array_equal(first, want[:64])
    assert not (second == want[64:]).all(axis=1).any()
    assert distinct(np.concatenate([first, second]))
    # without the knob the same two calls continue one stream (the default interval is 2^32)
    monkeypatch.delenv("QGCM_NONCE_RESEED")
    ctx2 = make_ctx()
    seed(ctx2, GEN_KEY, v0)
    both = np.concatenate([fill(torch, ctx2, 64).cpu().numpy(), fill(torch, ctx2, 64).cpu().numpy()]).reshape(128, 12)
    assert np.array_equal(both, want)


# ---- 9. the compression chain does not take the marker ----

def test_compress_seal_host_refuses_generate(torch, make_ctx):
    from quantum_amd import _lib

    ctx = make_ctx()
    ctx.set_key(0, bytes(range(32)))
    seed(ctx, GEN_KEY, 9)
    n, stride = 32, 1472
    rng = np.random.default_rng(0x90D3)
    arena, aptr, free = host_buffer(n * stride, True)
    try:
        arena[:] = rng.integers(0, 256, n * stride, dtype=np.uint8)
        plain = arena.copy()
        lens = rng.integers(1, 1400, n).astype(np.uint32)
        lens0 = lens.copy()
        status = np.full(n, 7, np.uint8)
        rc = _lib.lib().qgcm_compress_seal_host(ctx.handle, aptr, stride, n, lens.ctypes.data, 0, _lib.NONCES_GENERATE,
                                                4, 4, status.ctypes.data)
        assert rc == _lib.QGCM_E_ARG
        assert np.array_equal(arena, plain) and np.array_equal(lens, lens0) and status.tolist() == [7] * n
        # and it drew nothing: the generator is still at position 0
        assert np.array_equal(fill(torch, ctx, 3).cpu().numpy().reshape(3, 12), stream(GEN_KEY, 9, 3))
    finally:
        del arena
        free()
