"""Every public routed host pipeline once, in two chunks (257 slots of 1 MiB), on one context, for a trace of what
each call enqueues (tools/trace_sequence.py): before call k (from 0) come k + 1 launches of a torch sign kernel,
which no pipeline has, so the trace shows where each call starts.  Writes a SHA-256 of every call's outputs (return
value, lengths, peers, statuses, tables, packed bytes, the defined bytes of every slot), so two builds can be
compared on what they compute as well.  The inputs are those of
tests/test_gpu_route_shared.py::test_one_context_serves_every_pipeline_form_in_turn.

    rocprofv3 --kernel-trace --memory-copy-trace --output-format csv -d <dir> -o t -- \
        python3 tools/route_forms.py <another libqgcm.so, or ''> <digest.json>
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np

from quantum_amd import _lib

if sys.argv[1]:
    _lib.LIB_PATH = os.path.abspath(sys.argv[1])

import torch

import gso_model as GM
import test_gpu_gro as G
from quantum_amd import route
from test_gpu_chain_route import BOTH, STRANGER, addr
from test_gpu_gso import host_segmented
from test_gpu_route_shared import MIB, TWO, coalesced_of

rng = np.random.default_rng(0x5A4ED)
dsts = (addr(3), addr(11), addr(7), STRANGER)
items = ([GM.tcp_frame(rng, 44 * 60 + 13, 60, dsts[i % 2]) for i in range(4)] +
         [GM.udp_frame(rng, 10 * 50 + 1, 50, dsts[(i + 1) % 4]) for i in range(7)])
g_packed, g_len, g_frames, n = GM.layout(items, 21)
assert n == TWO
f_packed, f_len, f_table = host_segmented(g_packed, g_len, g_frames, n, 160)
nonces = rng.integers(0, 256, 12 * n, dtype=np.uint8)
helper = G.loop_ctx(3)
_, slots, s_lens, _, s_status = G.sealed_batch(helper, 3, 400, 0x5A4EE)
helper.close()
src = np.flatnonzero((s_status == 1) & (s_lens != 0))[:TWO]
dgrams = [slots[i, :int(s_lens[i])].copy() for i in src]
dgrams[7][40] ^= 1
dgrams[19][0:4] = np.frombuffer(STRANGER.to_bytes(4, "little"), np.uint8)
d_len = np.array([len(d) for d in dgrams], np.uint32)
packed, used, bufs = coalesced_of(dgrams)
# plain-sealed datagrams for the two plain opens come from the plain seal below
arena = np.zeros(TWO * MIB, np.uint8)
heads = arena.reshape(TWO, MIB)[:, :2048]
p_len = f_table[:, 1].astype(np.uint32)


def packets_in():
    for j in range(TWO):
        o, L = int(f_table[j, 0]), int(f_table[j, 1])
        heads[j, 4:4 + L] = f_packed[o:o + L]
    return p_len.copy()


def dgrams_in(ds):
    for j, d in enumerate(ds):
        heads[j, :len(d)] = d
    return np.array([len(d) for d in ds], np.uint32)


def outs():
    return np.full(TWO, 7, np.uint32), np.full(TWO, 0xAB, np.uint8)


def defined(lens, status, fallback):
    return [heads[j, :(4 + int(lens[j])) if status[j] == 1 else int(fallback[j])].copy() for j in range(TWO)]


c = G.loop_ctx(3)
plain_sealed = {}
digests = {}


def record(name, *parts):
    h = hashlib.sha256()
    for p in parts:
        if isinstance(p, list):
            for q in p:
                h.update(np.ascontiguousarray(q).tobytes())
        else:
            h.update(np.ascontiguousarray(p).tobytes())
    digests[name] = h.hexdigest()
    print(name, digests[name][:16], flush=True)


def seal_plain():
    lens = packets_in()
    peer, status = outs()
    rc = route.route_seal_host(c, arena.ctypes.data, MIB, TWO, lens, nonces.ctypes.data, peer, status)
    plain_sealed["d"] = [heads[j, :int(lens[j])].copy() for j in range(TWO) if status[j] == 1]
    record("route_seal_host", [rc], lens, peer, status, [heads[j, :int(lens[j])] for j in range(TWO)])


def open_plain():
    ds = (plain_sealed["d"] * 3)[:TWO]
    lens = dgrams_in(ds)
    fall = lens.copy()
    peer, status = outs()
    rc = route.route_open_host(c, arena.ctypes.data, MIB, TWO, lens, peer, status)
    record("route_open_host", [rc], lens, peer, status, defined(lens, status, fall))


def chain_seal():
    lens = packets_in()
    peer, status = outs()
    rc = route.route_chain_seal_host(c, arena.ctypes.data, MIB, TWO, lens, nonces.ctypes.data, BOTH, peer, status)
    record("route_chain_seal_host", [rc], lens, peer, status, [heads[j, :int(lens[j])] for j in range(TWO)])


def chain_open():
    lens = dgrams_in(dgrams)
    peer, status = outs()
    rc = route.route_chain_open_host(c, arena.ctypes.data, MIB, TWO, lens, BOTH, peer, status)
    record("route_chain_open_host", [rc], lens, peer, status, defined(lens, status, d_len))


def open_gro():
    ds = (plain_sealed["d"] * 3)[:TWO]
    pk, us, bf = coalesced_of(ds)
    lens = np.zeros(TWO, np.uint32)
    peer, status = outs()
    rc = route.route_open_gro_host(c, pk, us, bf, arena.ctypes.data, MIB, TWO, lens, peer, status)
    record("route_open_gro_host", [rc], lens, peer, status, defined(lens, status, np.array([len(d) for d in ds])))


def chain_open_gro():
    lens = np.zeros(TWO, np.uint32)
    peer, status = outs()
    rc = route.route_chain_open_gro_host(c, packed, used, bufs, arena.ctypes.data, MIB, TWO, lens, BOTH, peer, status)
    record("route_chain_open_gro_host", [rc], lens, peer, status, defined(lens, status, d_len))


def packed_open(name, call, gro):
    def run():
        lens = np.zeros(TWO, np.uint32) if gro else dgrams_in(dgrams)
        peer, status = outs()
        out_buf = np.zeros(1 << 19, np.uint8)
        if gro:
            rc, table, out = call(c, packed, used, bufs, MIB, TWO, lens, BOTH, peer, status, out_buf)
        else:
            rc, table, out = call(c, arena.ctypes.data, MIB, TWO, lens, BOTH, peer, status, out_buf)
        assert int(out[0]) == TWO
        record(name, [rc], lens, peer, status, table, out, out_buf[:int(out[2])])
    return run


def packed_seal(name, call, table):
    def run():
        lens = packets_in() if table is None else np.zeros(TWO, np.uint32)
        peer, status = outs()
        out_buf = np.zeros(1 << 17, np.uint8)
        ptrains, order = np.zeros((TWO, 4), np.uint32), np.zeros(TWO, np.uint32)
        if table is None:
            rc, pt, od, out = call(c, arena.ctypes.data, MIB, TWO, lens, nonces.ctypes.data, BOTH, peer, status, out_buf, None,
                                   ptrains, order)
        else:
            rc, pt, od, out = call(c, *table, MIB, TWO, lens, nonces.ctypes.data, BOTH, peer, status, out_buf, None, ptrains, order)
        assert int(out[0]) == TWO
        record(name, [rc], lens, peer, status, pt, od, out, out_buf[:int(out[2])])
    return run


calls = [seal_plain, open_plain, chain_seal, chain_open, open_gro, chain_open_gro,
         packed_open("route_chain_open_packed_host", route.route_chain_open_packed_host, False),
         packed_open("route_chain_open_gro_packed_host", route.route_chain_open_gro_packed_host, True),
         packed_open("route_chain_open_coalesced_host", route.route_chain_open_coalesced_host, False),
         packed_open("route_chain_open_gro_coalesced_host", route.route_chain_open_gro_coalesced_host, True),
         packed_seal("route_chain_seal_packed_host", route.route_chain_seal_packed_host, None),
         packed_seal("route_chain_seal_frames_host", route.route_chain_seal_frames_host, (f_packed, f_len, f_table)),
         packed_seal("route_chain_seal_gso_host", route.route_chain_seal_gso_host, (g_packed, g_len, g_frames))]
mark = torch.ones(64, device="cuda")
for k, call in enumerate(calls):
    for _ in range(k + 1):  # the marker in the trace: k + 1 launches of a kernel no pipeline has
        torch.sign(mark)
    torch.cuda.synchronize()
    call()
for _ in range(len(calls) + 1):
    torch.sign(mark)
torch.cuda.synchronize()
c.close()
with open(sys.argv[2], "w") as f:
    json.dump(digests, f, indent=1)
    f.write("\n")
