"""Every open path against the forged-record matrix of forgery_cases.py.

Each case opens a batch in which every odd packet carries exactly one forgery (every bit of a short
record; header, tag, nonce and block-edge bits of long ones; one tag bit for every L mod 16 against every
nfull mod 4; spliced tags, nonces and ciphertexts; another valid key; a sealed length off by 1 or 16)
between authentic neighbours, and asserts that the status array (junk 0x5A before the call) and the WHOLE
arena, gaps included, equal what O.aesgo_open_descs leaves, and that the kernel the case is named after
took the batch (qgcm_launch_counts).  Paths: the uniform quad kernel at both slot alignments, the default
uniform dispatch on either side of its 2048-packet threshold, the per-wave and the segmented descriptor
kernels, gcm_one_kernel reading descriptors (a one-member group's direct path), per-packet Decrypt on the
resident and on the launch path, and the tiles the uniform kernel hands out from its global counter."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import forgery_cases as FC
from oracle import oracle as O

pytestmark = pytest.mark.gpu

NKEYS = 32
KEYS = np.random.default_rng(0xF02CE).bytes(32 * NKEYS)
KNOBS = ("QGCM_VARIANT", "QGCM_DESC_VARIANT", "QGCM_RESIDENT")
KERNELS = ("quad", "segmented", "per_wave", "one", "resident")
SEG_MIN_PACKETS = 753  # (kSegMinTiles - 1) * 16 + 1: a key with this many packets is a segmented-kernel run


@pytest.fixture(scope="module")
def torch():
    import torch as T

    if not T.cuda.is_available():
        pytest.skip("no GPU")
    return T


@pytest.fixture(scope="module")
def ctxs(torch):
    """One context per knob setting (the knobs are read at qgcm_create), all with the same key table."""
    from quantum_amd.crypto import Context

    settings = {"quad": {"QGCM_VARIANT": "12"}, "default": {}, "per_wave": {"QGCM_DESC_VARIANT": "13"},
                "launch": {"QGCM_RESIDENT": "0"}}
    saved = {k: os.environ.get(k) for k in KNOBS}
    out = {}
    try:
        for name, env in settings.items():
            for k in KNOBS:
                os.environ.pop(k, None)
            os.environ.update(env)
            out[name] = Context(device=0, max_keys=64)
            out[name].set_keys(0, KEYS)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    yield out
    for c in out.values():
        c.close()


class Counted:
    """The launches a context counted inside the block, per kernel."""

    def __init__(self, torch, ctx):
        self.torch, self.ctx, self.delta = torch, ctx, None

    def __enter__(self):
        self.before = self.ctx.launch_counts()
        return self

    def __exit__(self, *exc):
        self.torch.cuda.synchronize()
        after = self.ctx.launch_counts()
        self.delta = {k: after[k] - self.before[k] for k in after}

    def only(self, **want):
        assert {k: self.delta[k] for k in KERNELS} == {k: want.get(k, 0) for k in KERNELS}, self.delta


@functools.lru_cache(maxsize=None)
def _uniform_cases(aad_len):
    """Per payload length, the uniform-stride batch (stride a multiple of 64) and what the oracle leaves."""
    specs = FC.full_matrix(with_descriptor_kinds=False) if aad_len == 4 else FC.short_matrix()
    out = {}
    for L, group in sorted(FC.uniform_groups(specs).items()):
        b = FC.build(KEYS, [5], group, seed=100 + L, aad_len=aad_len, uniform=True, align=64)
        out[L] = (b,) + FC.oracle_open(b)
    return out


@functools.lru_cache(maxsize=None)
def _desc_case(name, aad_len=4):
    if aad_len != 4:  # the short records, every bit; 4-B-aligned records on a few keys, one of them a long run
        specs = [s if i % 3 else FC.replace(s, key=1 + i % 4) for i, s in enumerate(FC.short_matrix())]
        b = FC.build(KEYS, [9, 3, 4, 5, 6], specs, seed=30 + aad_len, aad_len=aad_len, base=4)
    elif name == "per_wave":  # the whole mixed-length matrix over a handful of keys, records at 4 mod 16
        b = FC.build(KEYS, [2, 3, 5, 7, 11], FC.on_keys(FC.full_matrix(), 5), seed=21, base=4)
    elif name == "segmented":  # every bit of the short records on ONE key (a run), the rest on 16 short-run keys
        rest = [s for L in FC.LONG_LENGTHS for s in FC.bit_long_specs(L)]
        rest += FC.residue_specs() + FC.field_specs() + FC.key_specs() + FC.length_specs()
        b = FC.build(KEYS, range(8, 25), FC.short_matrix() + FC.on_keys(rest, 16, first=1), seed=22, base=4)
    elif name == "descs_one":  # small keyed batch, 16-B-aligned records
        b = FC.build(KEYS, [1, 2, 3], FC.on_keys(FC.residue_specs() + FC.field_specs(), 3), seed=23)
    elif name == "per_packet":
        b = FC.build(KEYS, [6], FC.bit_specs(0) + FC.bit_specs(17) + FC.residue_specs(), seed=24)
    else:
        raise KeyError(name)
    return (b,) + FC.oracle_open(b)


def _open_uniform(torch, ctx, b, lead):
    """The uniform batch opened with its arena `lead` bytes into a 256-B-aligned allocation."""
    from quantum_amd import batch

    alloc = torch.zeros(lead + len(b.arena) + 64, dtype=torch.uint8, device="cuda")
    arena = alloc[lead:lead + len(b.arena)]
    arena.copy_(torch.from_numpy(b.arena))
    status = torch.full((b.n,), 0x5A, dtype=torch.uint8, device="cuda")
    batch.open_uniform(ctx, arena, b.stride, b.n, int(b.lens[0]), int(b.kidx[0]), aad_len=b.aad_len, status=status)
    assert not alloc[:lead].any() and not alloc[lead + len(b.arena):].any()
    return status.cpu().numpy(), arena.cpu().numpy()


def _run_uniform_cases(torch, ctx, aad_len, lead, kernel):
    failed = []
    for L, (b, want_st, want_arena) in _uniform_cases(aad_len).items():
        with Counted(torch, ctx) as c:
            st, arena = _open_uniform(torch, ctx, b, lead)
        c.only(**{kernel: 1})
        bad = FC.mismatches(b, st, arena, want_st, want_arena)
        if bad:
            failed.append(f"L={L}: {bad}")
    assert not failed, f"{len(failed)} lengths differ from the oracle:\n" + "\n".join(failed[:12])


@pytest.mark.parametrize("aad_len,lead", [(4, 0), (4, 60), (0, 0), (1, 60), (3, 0)])
def test_uniform_quad_kernel(torch, ctxs, aad_len, lead):
    """QGCM_VARIANT=12: one call per payload length (99 lengths with the 4-byte header as additional data;
    every bit of the short records with 0, 1 and 3 bytes of it), with the arena 16-B aligned and at 60 mod
    64, where read_tag and the tail take their unaligned forms."""
    _run_uniform_cases(torch, ctxs["quad"], aad_len, lead, "quad")


@pytest.mark.parametrize("aad_len", [4, 0, 1, 3])
def test_uniform_default_small_batches(torch, ctxs, aad_len):
    """Default dispatch: at most 2048 16-B-aligned slots run gcm_one_kernel, one workgroup a packet."""
    assert max(b.n for b, _, _ in _uniform_cases(aad_len).values()) <= 2048
    _run_uniform_cases(torch, ctxs["default"], aad_len, 0, "one")


def test_uniform_default_past_2048_packets(torch, ctxs):
    """Default dispatch: every bit of the L = 17 record three times over, 2353 packets, runs the quad kernel."""
    b = FC.build(KEYS, [5], FC.bit_specs(17) * 3, seed=40, uniform=True)
    assert b.n == 2353 > 2048
    want_st, want_arena = FC.oracle_open(b)
    with Counted(torch, ctxs["default"]) as c:
        st, arena = _open_uniform(torch, ctxs["default"], b, 0)
    c.only(quad=1)
    bad = FC.mismatches(b, st, arena, want_st, want_arena)
    assert not bad, bad


def _open_descs(torch, ctx, b):
    from quantum_amd import batch

    arena = torch.from_numpy(b.arena).cuda()
    status = torch.full((b.n,), 0x5A, dtype=torch.uint8, device="cuda")
    batch.open_batch(ctx, arena, batch.make_descs(b.offs, b.lens, b.kidx, "cuda"), b.n, aad_len=b.aad_len,
                     status=status)
    return status.cpu().numpy(), arena.cpu().numpy()


@pytest.mark.parametrize("aad_len", [4, 0, 1, 3])
def test_descriptor_per_wave_kernel(torch, ctxs, aad_len):
    """QGCM_DESC_VARIANT=13: the whole matrix, `key` and `length` kinds included, in one batch over five
    keys, records at 4 mod 16."""
    b, want_st, want_arena = _desc_case("per_wave" if aad_len == 4 else "short", aad_len)
    assert all(int(o) % 16 == 4 for o in b.offs)
    if aad_len == 4:
        assert {k: int((b.kind == k).sum()) for k in FC.COUNTS} == FC.COUNTS
    with Counted(torch, ctxs["per_wave"]) as c:
        st, arena = _open_descs(torch, ctxs["per_wave"], b)
    c.only(per_wave=1)
    bad = FC.mismatches(b, st, arena, want_st, want_arena)
    assert not bad, bad


@pytest.mark.parametrize("aad_len", [4, 0, 1, 3])
def test_descriptor_segmented_kernel(torch, ctxs, aad_len):
    """Default descriptor variant: the `bit` matrix on one key whose run the segmented kernel takes, the
    other kinds on keys too short for a run, which its per-wave pass takes."""
    b, want_st, want_arena = _desc_case("segmented" if aad_len == 4 else "short", aad_len)
    per_key = np.bincount(b.kidx)
    run_key = int(np.argmax(per_key))
    assert per_key[run_key] >= SEG_MIN_PACKETS
    assert (np.delete(per_key, run_key) < SEG_MIN_PACKETS).all() and (per_key > 0).sum() > 1
    if aad_len == 4:
        assert (b.kidx[b.kind == "bit"] == run_key).all() and (b.kidx[(b.kind != "bit") & b.forged] != run_key).all()
        assert {k: int((b.kind == k).sum()) for k in FC.COUNTS} == FC.COUNTS
    with Counted(torch, ctxs["default"]) as c:
        st, arena = _open_descs(torch, ctxs["default"], b)
    c.only(segmented=1, per_wave=1)
    bad = FC.mismatches(b, st, arena, want_st, want_arena)
    assert not bad, bad


def test_descriptor_one_workgroup_per_packet(torch):
    """run_descs_one (gcm_one_kernel reading descriptors): a one-member group opens a small keyed batch of
    16-B-aligned records in place in a pinned arena; the `residue` and `field` kinds."""
    from quantum_amd import _lib, shard

    b, want_st, want_arena = _desc_case("descs_one")
    assert all(int(o) % 16 == 0 for o in b.offs) and b.n <= 8192  # kDescOneMax
    grp = shard.Group([0], max_keys=64)
    ptr = _lib.lib().qgcm_host_alloc(len(b.arena))
    try:
        assert ptr
        grp.set_keys(0, KEYS)
        ctx = grp.member(0)
        arena = np.frombuffer((C.c_uint8 * len(b.arena)).from_address(ptr), dtype=np.uint8)
        arena[:] = b.arena
        status = np.full(b.n, 0x5A, np.uint8)
        with Counted(torch, ctx) as c:
            bad = grp.open_host(ptr, shard.host_descs(b.offs, b.lens, b.kidx), b.n, 4, status.ctypes.data)
        c.only(one=1)
        assert grp.last_path(0) == "direct"
        diff = FC.mismatches(b, status, arena, want_st, want_arena)
        assert not diff, diff
        assert bad == int((want_st == 0).sum())
        del arena
    finally:
        _lib.lib().qgcm_host_free(ptr)
        grp.close()


@functools.lru_cache(maxsize=None)
def _per_packet_expected():
    """crypto/aes.go:57-62 on every record of the per-packet batch: (record, additional data, what
    O.aesgo_decrypt leaves, its return value)."""
    b, _, _ = _desc_case("per_packet")
    out = []
    for i in range(b.n):
        rec = bytes(b.record(i))
        o = int(b.offs[i])
        aad = bytes(b.arena[o:o + 4])
        want = bytearray(rec)
        rc = O.aesgo_decrypt(KEYS[32 * int(b.kidx[i]):32 * int(b.kidx[i]) + 32], want, aad)
        out.append((rec, aad, bytes(want), rc))
    return b, out


@pytest.mark.parametrize("path,kernel", [("default", "resident"), ("launch", "one")])
def test_per_packet_decrypt(torch, ctxs, path, kernel):
    """(*AES).Decrypt on every record, one call each: every bit of the L = 0 and L = 17 records and the
    `residue` set, through the resident kernel and, with QGCM_RESIDENT=0, a gcm_one_kernel launch per call.
    A forged record returns the error with [0, L) zeroed and tag and nonce untouched."""
    from quantum_amd.crypto import AES

    b, expected = _per_packet_expected()
    assert sum(rc < 0 for _, _, _, rc in expected) == 8 * 32 + 8 * 49 + 96
    ctx = ctxs[path]
    aes = AES(KEYS[32 * int(b.kidx[0]):32 * int(b.kidx[0]) + 32], ctx=ctx)
    failed = []
    with Counted(torch, ctx) as c:
        for i, (rec, aad, want, rc) in enumerate(expected):
            data = bytearray(rec)
            n, err = aes.Decrypt(data, aad)
            L = len(rec) - FC.OVERHEAD
            if (err is None) != (rc >= 0) or n != L or bytes(data) != want:
                zeroed = bytes(data[:L]) == bytes(L)
                failed.append(f"{b.describe(i)}: err {err!r} (oracle returns {rc}), plaintext "
                              f"{'zeroed' if zeroed else 'not zeroed'}, tail {'kept' if bytes(data[L:]) == rec[L:] else 'changed'}")
    c.only(**{kernel: b.n})
    assert not failed, f"{len(failed)} records differ from the oracle:\n" + "\n".join(failed[:12])


def test_shared_tail_rejects_forged_records(torch, ctxs):
    """Two full rows of tiles and a ragged one (L = 33, stride 80): the second row and the ragged tiles come
    from the launch's global counter.  64 forged packets, each with another tag bit flipped: the first and
    last packet of the first row, of the counter's row and of the launch, the ragged last tile's first,
    middle and last packet, both neighbours of tile, wave-row and workgroup boundaries, the rest seeded."""
    from quantum_amd import batch

    ctx = ctxs["default"]
    L, stride = 33, 80
    rp = torch.cuda.get_device_properties(0).multi_processor_count * 2 * 16 * 16  # one row of tiles, in packets
    n = 2 * rp + 4096 + 11
    last_tile = (n - 1) // 16 * 16
    assert n - last_tile == 11
    rng = np.random.default_rng(0x7A11F0)
    forged = [0, rp - 1, rp, 2 * rp - 1, 2 * rp, n - 1, last_tile, last_tile + 5,
              rp + 16 * 1000 - 1, rp + 16 * 1000, rp + 256 * 77 - 1, rp + 256 * 77, 2 * rp + 16 * 9 - 1, 2 * rp + 16 * 9,
              15, 16]
    pool = np.setdiff1d(np.arange(n), forged)
    forged = np.array(forged + rng.choice(pool, 64 - len(forged), replace=False).tolist())
    assert len(set(forged.tolist())) == 64

    arena = rng.integers(0, 256, n * stride, dtype=np.uint8)
    offs = np.arange(n, dtype=np.uint64) * stride
    kidx = np.full(n, 5, dtype=np.uint32)
    O.aesgo_seal_descs(KEYS, arena, offs, np.full(n, L, np.uint32), kidx,
                       rng.integers(0, 256, 12 * n, dtype=np.uint8), 4, 8)
    for j, i in enumerate(forged):  # tag bit 2 j: every tag byte, all four words
        arena[int(i) * stride + 4 + L + (2 * j >> 3)] ^= 1 << (2 * j & 7)
    want_arena = arena.copy()
    want_st = np.full(n, 0x5A, np.uint8)
    O.aesgo_open_descs(KEYS, want_arena, offs, np.full(n, L + 28, np.uint32), kidx, want_st, 4, 8)
    want = np.ones(n, np.uint8)
    want[forged] = 0
    assert np.array_equal(want_st, want)

    d_arena = torch.from_numpy(arena).cuda()
    status = torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda")
    with Counted(torch, ctx) as c:
        batch.open_uniform(ctx, d_arena, stride, n, L + 28, 5, status=status)
    c.only(quad=1)
    assert c.delta["tail_waits"] == 0
    st = status.cpu().numpy()
    wrong = np.flatnonzero(st != want_st)
    assert not len(wrong), f"{len(wrong)} statuses differ, first packets {wrong[:8].tolist()} of {n} (row {rp})"
    got = d_arena.cpu().numpy()
    if not np.array_equal(got, want_arena):
        slots = np.flatnonzero((got != want_arena).reshape(n, stride).any(axis=1))
        pytest.fail(f"{len(slots)} slots differ from the oracle, first {slots[:8].tolist()} of {n} (row {rp}); "
                    f"forged: {sorted(set(slots.tolist()) & set(forged.tolist()))[:8]}")
