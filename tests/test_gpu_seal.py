"""Every seal path against the matrix of seal_cases.py.

Each case seals a batch whose arena is random in EVERY byte (headers, payloads, the 28 bytes tag and nonce
go to, gaps, the lead before slot 0, the bytes behind the last slot) and asserts that the status array
(junk 0x5A before the call) and the WHOLE arena equal what O.aesgo_seal_descs leaves, and that the kernel
the case is named after took the batch (qgcm_launch_counts).  The lengths are every residue mod 64 twice
(0..130), every block count up to 68, and the boundaries of the one-workgroup kernel, the counter's second
byte and the staging rows (seal_cases.py says which and why); the uniform layouts put slots at every offset
mod 16, down to the minimal stride where a record's last dword ends at the next slot's header; the nonce
comes from an array at 4 mod 16 or from the slot.  Paths: the uniform quad kernel (QGCM_VARIANT=12), the
default uniform dispatch with a case for every reason it refuses the one-workgroup kernel, that kernel
without flat GHASH tables, the per-wave and the segmented descriptor kernels, gcm_one_kernel reading
descriptors (a one-member group's direct path) and per-packet Encrypt on the resident and the launch path.

Seal forms that stay outside, and the file that covers each: nonces drawn on the GPU
(QGCM_NONCES_GENERATE) test_gpu_nonce.py; chunked launches test_gpu_parity.py::test_uniform_chunked_launches
(QGCM_LAUNCH_CHUNK) and test_gpu_nonce.py::test_seal_batch_generate (QGCM_DESC_CHUNK); the tiles a large
launch hands out from its global counter (the shared tail) test_gpu_tail_pool.py; rejected packets (key slot
unset or out of range, payload too long) test_gpu_desc_edges.py and
test_gpu_parity.py::test_descriptor_batch_bad_key_and_short, ::test_payload_limit_rejected."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import seal_cases as SC
from oracle import oracle as O

pytestmark = pytest.mark.gpu

KNOBS = ("QGCM_VARIANT", "QGCM_DESC_VARIANT", "QGCM_RESIDENT", "QGCM_FLAT_GHASH_KEYS")
KERNELS = ("quad", "segmented", "per_wave", "one", "resident")


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
                "launch": {"QGCM_RESIDENT": "0"}, "noflat": {"QGCM_FLAT_GHASH_KEYS": "0"}}
    saved = {k: os.environ.get(k) for k in KNOBS}
    out = {}
    try:
        for name, env in settings.items():
            for k in KNOBS:
                os.environ.pop(k, None)
            os.environ.update(env)
            out[name] = Context(device=0, max_keys=64)
            out[name].set_keys(0, SC.KEYS)
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
def _expected(make, *args):
    """(batch, oracle status, oracle arena) of a seal_cases.py case, worked out once a session."""
    b = make(*args)
    return (b,) + SC.oracle_seal(b)


def _device_nonces(torch, b):
    """The nonce array at 4 mod 16 (the calls ask for 4-B alignment only); None: the nonce is in the slot."""
    if b.nonces is None:
        return None
    buf = torch.zeros(4 + len(b.nonces), dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf[4:].copy_(torch.from_numpy(b.nonces))
    return buf[4:]


def _seal_uniform(torch, ctx, b, with_status=True):
    """The uniform batch sealed in a 256-B-aligned allocation that holds the arena's lead, slots and trail."""
    from quantum_amd import batch

    alloc = torch.from_numpy(b.arena).cuda()
    assert alloc.data_ptr() % 256 == 0
    status = torch.full((b.n,), 0x5A, dtype=torch.uint8, device="cuda") if with_status else None
    batch.seal_uniform(ctx, alloc[b.lead:], b.stride, b.n, int(b.lens[0]), int(b.kidx[0]), _device_nonces(torch, b),
                       aad_len=b.aad_len, status=status)
    return (status.cpu().numpy() if with_status else None), alloc.cpu().numpy()


def _run_uniform(torch, ctx, cases, kernel, with_status=True):
    """cases: (label, batch, oracle status, oracle arena), one call each; fails once, with the first dozen."""
    failed = []
    for label, b, want_st, want_arena in cases:
        with Counted(torch, ctx) as c:
            st, arena = _seal_uniform(torch, ctx, b, with_status)
        c.only(**{kernel: 1})
        bad = SC.mismatches(b, st, arena, want_st, want_arena)
        if bad:
            failed.append(f"{label}: {bad}")
    assert not failed, f"{len(failed)} of {len(cases)} calls differ from the oracle:\n" + "\n".join(failed[:12])


def _quad_cases(config, aad_len, lengths):
    return [(f"L={L}",) + _expected(SC.quad_case, L, config, aad_len) for L in lengths]


@pytest.mark.parametrize("config", list(SC.QUAD_CONFIGS))
def test_uniform_quad_kernel(torch, ctxs, config):
    """QGCM_VARIANT=12, every length, 37 packets a call: 16-B-aligned slots with a nonce array; the minimal
    stride (slots at every offset mod 16, no gap but the 4-B rounding) with the nonce in the slot, 60 bytes
    into the allocation, and with a nonce array; a stride of 4 mod 16 with the nonce in the slot."""
    _run_uniform(torch, ctxs["quad"], _quad_cases(config, 4, SC.SEAL_LENGTHS), "quad")


@pytest.mark.parametrize("aad_len", [0, 1, 3])
def test_uniform_quad_kernel_short_additional_data(torch, ctxs, aad_len):
    """0..130 at the minimal stride, nonce in the slot, with 0, 1 and 3 bytes of the header as additional data."""
    _run_uniform(torch, ctxs["quad"], _quad_cases("min4_slot", aad_len, SC.SHORT), "quad")


def test_uniform_quad_kernel_without_status(torch, ctxs):
    """The minimal-stride, nonce-in-slot configuration again with status = NULL."""
    _run_uniform(torch, ctxs["quad"], _quad_cases("min4_slot", 4, SC.SEAL_LENGTHS), "quad", with_status=False)


def _one_cases(stride, from_slot, lengths):
    return [(f"L={L}",) + _expected(SC.one_case, L, stride, from_slot) for L in lengths if L <= SC.ONE_CAP_LEN]


@pytest.mark.parametrize("from_slot", [False, True], ids=["array", "slot"])
@pytest.mark.parametrize("stride", ["s16", "s16p16"])
def test_uniform_default_one_workgroup_kernel(torch, ctxs, stride, from_slot):
    """Default dispatch, 5 packets a call: slots exactly as long as gcm_one_kernel's staging area, and 16
    bytes longer (the row behind the staged ones must stay as it was), up to L = 32720, the longest it takes."""
    cases = _one_cases(stride, from_slot, SC.SEAL_LENGTHS)
    assert len(cases) == len(SC.SEAL_LENGTHS) - 1
    _run_uniform(torch, ctxs["default"], cases, "one")


def test_uniform_default_dispatch_to_quad_kernel(torch, ctxs):
    """One case per reason run_uniform refuses the one-workgroup kernel -- a stride that is no multiple of
    16, an arena at 4 mod 16, a record past the staging area -- and 2049 packets, nonce in the slot with
    L % 4 != 0 (read_nonce's byte loads in the quad kernel): all the quad kernel's, all the oracle's bytes."""
    cases = [(name,) + _expected(SC.dispatch_case, name) for name in SC.DISPATCH]
    assert {b.n for _, b, _, _ in cases} == {3, 5, 2049}
    _run_uniform(torch, ctxs["default"], cases, "quad")


def test_uniform_one_workgroup_kernel_without_flat_tables(torch, ctxs):
    """QGCM_FLAT_GHASH_KEYS=0: the Horner + Estrin GHASH from the comb tables in LDS at every count of tables
    (0..130 and 16 k, 16 k + 1 up to 68 blocks)."""
    _run_uniform(torch, ctxs["noflat"], _one_cases("s16", True, SC.SHORT + SC.SERIES), "one")


def _seal_descs(torch, ctx, b):
    from quantum_amd import batch

    arena = torch.from_numpy(b.arena).cuda()
    status = torch.full((b.n,), 0x5A, dtype=torch.uint8, device="cuda")
    batch.seal_batch(ctx, arena, batch.make_descs(b.offs, b.lens, b.kidx, "cuda"), b.n, _device_nonces(torch, b),
                     aad_len=b.aad_len, status=status)
    return status.cpu().numpy(), arena.cpu().numpy()


@pytest.mark.parametrize("aad_len", [4, 0])
@pytest.mark.parametrize("from_slot", [False, True], ids=["array", "slot"])
def test_descriptor_per_wave_kernel(torch, ctxs, from_slot, aad_len):
    """QGCM_DESC_VARIANT=13: every length below 9001 in one batch over five keys, records packed at 4 B
    from offset 4 with gaps of 0, 4 and 8 bytes."""
    b, want_st, want_arena = _expected(SC.per_wave_case, from_slot, aad_len)
    with Counted(torch, ctxs["per_wave"]) as c:
        st, arena = _seal_descs(torch, ctxs["per_wave"], b)
    c.only(per_wave=1)
    bad = SC.mismatches(b, st, arena, want_st, want_arena)
    assert not bad, bad


@pytest.mark.parametrize("from_slot", [False, True], ids=["array", "slot"])
def test_descriptor_segmented_kernel(torch, ctxs, from_slot):
    """Default descriptor variant: every length below 9001 on one key with 753 packets, a run the segmented
    kernel takes, and 0..130 on 16 keys too short for a run, which its per-wave pass takes."""
    b, want_st, want_arena = _expected(SC.segmented_case, from_slot)
    per_key = np.bincount(b.kidx)
    run_key = int(np.argmax(per_key))
    assert per_key[run_key] >= SC.SEG_MIN_PACKETS
    assert (np.delete(per_key, run_key) < SC.SEG_MIN_PACKETS).all() and (per_key > 0).sum() == 17
    with Counted(torch, ctxs["default"]) as c:
        st, arena = _seal_descs(torch, ctxs["default"], b)
    c.only(segmented=1, per_wave=1)
    bad = SC.mismatches(b, st, arena, want_st, want_arena)
    assert not bad, bad


@pytest.mark.parametrize("from_slot", [False, True], ids=["array", "slot"])
def test_descriptor_one_workgroup_per_packet(torch, from_slot):
    """run_descs_one (gcm_one_kernel reading descriptors): a one-member group seals 0..130 and the
    one-kernel boundary lengths in place in a pinned arena, 16-B-aligned records over three keys."""
    from quantum_amd import _lib, shard

    b, want_st, want_arena = _expected(SC.descs_one_case, from_slot)
    assert all(int(o) % 16 == 0 for o in b.offs) and b.n <= 8192  # kDescOneMax
    grp = shard.Group([0], max_keys=64)
    ptr = _lib.lib().qgcm_host_alloc(len(b.arena))
    try:
        assert ptr
        grp.set_keys(0, SC.KEYS)
        ctx = grp.member(0)
        arena = np.frombuffer((C.c_uint8 * len(b.arena)).from_address(ptr), dtype=np.uint8)
        arena[:] = b.arena
        status = np.full(b.n, 0x5A, np.uint8)
        nonces = None if b.nonces is None else b.nonces.ctypes.data
        with Counted(torch, ctx) as c:
            bad = grp.seal_host(ptr, shard.host_descs(b.offs, b.lens, b.kidx), b.n, nonces, 4, status.ctypes.data)
        c.only(one=1)
        assert grp.last_path(0) == "direct"
        diff = SC.mismatches(b, status, arena, want_st, want_arena)
        assert not diff, diff
        assert bad == 0
        del arena
    finally:
        _lib.lib().qgcm_host_free(ptr)
        grp.close()


@functools.lru_cache(maxsize=None)
def _per_packet_expected():
    """crypto/aes.go:41-52 by O.aesgo_encrypt on every per-packet buffer: random plaintext, random bytes where
    tag and nonce go and 8 more behind them; 0 and 4 bytes of additional data."""
    rng = np.random.default_rng(0x5EA1BEEF)
    out = []
    for L in SC.PER_PACKET_LENGTHS:
        for aad_len in (0, 4):
            buf, aad, nonce = rng.bytes(L + SC.OVERHEAD + 8), rng.bytes(aad_len), rng.bytes(12)
            want = bytearray(buf)
            assert O.aesgo_encrypt(SC.KEYS[:32], want, L, aad or None, nonce) == L + SC.OVERHEAD
            out.append((L, buf, aad, nonce, bytes(want)))
    return out


@pytest.mark.parametrize("path,kernel", [("default", "resident"), ("launch", "one")])
def test_per_packet_encrypt(torch, ctxs, path, kernel):
    """(*AES).Encrypt, one call a buffer, at the one-kernel boundaries and at every block count from 9 to 68,
    through the resident kernel and, with QGCM_RESIDENT=0, a gcm_one_kernel launch per call."""
    from quantum_amd.crypto import AES

    expected = _per_packet_expected()
    assert len(expected) == 2 * SC.COUNTS["per_packet"]
    ctx = ctxs[path]
    aes = AES(SC.KEYS[:32], ctx=ctx)  # takes the context's slot 0, which holds this key already
    failed = []
    with Counted(torch, ctx) as c:
        for L, buf, aad, nonce, want in expected:
            data = bytearray(buf)
            n, err = aes.Encrypt(data, L, aad or None, nonce=nonce)
            if err is not None or n != L + SC.OVERHEAD or bytes(data) != want:
                diff = [i for i in range(len(want)) if data[i] != want[i]]
                failed.append(f"L={L}, {len(aad)} bytes of additional data: err {err!r}, n {n}, "
                              f"{len(diff)} bytes differ from byte {diff[0] if diff else None}")
    c.only(**{kernel: len(expected)})
    assert not failed, f"{len(failed)} buffers differ from the oracle:\n" + "\n".join(failed[:12])
