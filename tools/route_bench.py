#!/usr/bin/env python3
"""Resolve and accounting launches beside the seal of the same batch and a host loop doing the same work.

2^20 slots of stride 1408 (1350-byte packets), 1024 peers.  Device figures are hipEvent times of one
launch, warm, the median of --reps repetitions (at least 20):
  * qgcm_resolve_outgoing,
  * qgcm_route_account with the peers uniform, and with 90 % of the packets on one link,
  * qgcm_seal_batch of the same batch (the nonce already in the slot).
Host figures are single-thread loops in this script over the same packets -- dict lookup, header write,
descriptor build: once as a plain interpreter loop, once vectorised with numpy (sorted-array lookup), the
kinder comparison.  Prints one JSON line, with the GPU's mean clock over the device timings.  The
comparison that matters is resolve and accounting against the seal launch and the host loops; a skewed
accounting run several times the uniform one would mean the on-chip combining is not working.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=1 << 20)
    ap.add_argument("--stride", type=int, default=1408)
    ap.add_argument("--peers", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--host-reps", type=int, default=3)
    args = ap.parse_args()
    reps = max(20, args.reps)
    import torch

    from quantum_amd import batch, route
    from quantum_amd.crypto import Context

    n, stride, peers, L = args.slots, args.stride, args.peers, args.stride - 58
    rng = np.random.default_rng(0x20B7E)
    ctx = Context(device=0, max_keys=peers)
    ctx.set_keys(0, rng.integers(0, 256, 32 * peers, dtype=np.uint8).tobytes())
    addrs = np.array([10 | 99 << 8 | (j >> 8) << 16 | (j & 255) << 24 for j in range(2, 2 + peers)], np.uint32)
    table = {int(a): k for k, a in enumerate(addrs)}
    net, mask, own = 10 | 99 << 8, 0xFFFF, 10 | 99 << 8 | 1 << 24
    gateway = 10 | 99 << 8 | 255 << 16 | 254 << 24
    route.routes_set(ctx, table, net, mask, gateway, own)
    mixes = {"uniform": rng.integers(0, peers, n), "skewed": np.where(rng.random(n) < 0.9, 7, rng.integers(0, peers, n))}
    arena = torch.zeros(n * stride, dtype=torch.uint8, device="cuda")
    lens = torch.full((n,), L, dtype=torch.int32, device="cuda")
    peer = torch.zeros(n, dtype=torch.int32, device="cuda")
    descs = torch.zeros(16 * n, dtype=torch.uint8, device="cuda")
    status = torch.zeros(n, dtype=torch.uint8, device="cuda")

    def set_dsts(mix):
        dst = torch.from_numpy(addrs[mixes[mix]].view(np.uint8).reshape(n, 4).copy()).cuda()
        arena.view(n, stride)[:, 20:24] = dst

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            out.append(a.elapsed_time(b) * 1e3)
        return statistics.median(out)

    res = {"slots": n, "stride": stride, "peers": peers, "reps": reps}
    from bench import GpuTelemetry  # the box's clock over the device timings, as bench.py reports it

    tel = GpuTelemetry(0)
    tel.span = "the device timings"
    tel.start()
    for mix in ("skewed", "uniform"):
        set_dsts(mix)
        us = timed(lambda: route.resolve_outgoing(ctx, arena, stride, n, lens, peer, descs))
        if mix == "uniform":
            res["resolve_outgoing_us"] = round(us, 1)
        assert np.array_equal(peer.cpu().numpy().view(np.uint32), mixes[mix].astype(np.uint32)), "resolve is wrong"
        status.fill_(1)
        res[f"account_{mix}_us"] = round(timed(lambda: route.route_account(ctx, route.TX, n, peer, descs, status)), 1)
    # the seal of the same batch (uniform peers), on the descriptors the resolve wrote
    res["seal_batch_us"] = round(timed(lambda: batch.seal_batch(ctx, arena, descs, n, None, status=status)), 1)
    tel.stop()
    res["sclk_mhz_mean"] = tel.summary().get("sclk_mhz_mean")
    # exactness of what the accounting launches added: 3 + reps launches per mix, every packet delivered
    tot = route.route_stats(ctx, route.TX)
    launches = 2 * (3 + reps)
    assert tot["Packets"] == launches * n and tot["Bytes"] == launches * n * (4 + L + 28), tot
    # the host doing the same: lookup, header write, descriptor build, one thread
    host = np.zeros(n * stride, np.uint8)
    dst_words = addrs[mixes["uniform"]]
    host.reshape(n, stride)[:, 20:24] = dst_words.view(np.uint8).reshape(n, 4)
    own_bytes = own.to_bytes(4, "little")

    def host_loop():
        mv = memoryview(host)
        out_peer, out_desc = [0] * n, [None] * n
        for i in range(n):
            o = i * stride
            d = int.from_bytes(mv[o + 20:o + 24], "little")
            p = table.get(d if (d & mask) == (net & mask) else gateway)
            if p is not None:
                mv[o:o + 4] = own_bytes
                out_peer[i] = p
                out_desc[i] = (o, L, p)
        return out_peer

    def host_numpy():
        order = np.argsort(addrs)
        sorted_addrs = addrs[order]
        h = host.reshape(n, stride)
        d = h[:, 20:24].copy().view(np.uint32).reshape(n)
        key = np.where((d & mask) == (net & mask), d, gateway).astype(np.uint32)
        pos = np.minimum(np.searchsorted(sorted_addrs, key), peers - 1)
        hit = sorted_addrs[pos] == key
        p = np.where(hit, order[pos], 0xFFFFFFFF).astype(np.uint32)
        h[hit, 0:4] = np.frombuffer(own_bytes, np.uint8)
        desc = np.zeros(n, np.dtype([("off", "<u8"), ("len", "<u4"), ("key", "<u4")]))
        desc["off"], desc["len"], desc["key"] = np.arange(n, dtype=np.uint64) * stride, L, p
        return p

    for name, fn in (("host_loop_us", host_loop), ("host_numpy_us", host_numpy)):
        ts = []
        for _ in range(max(1, args.host_reps)):
            t0 = time.perf_counter()
            got = fn()
            ts.append((time.perf_counter() - t0) * 1e6)
        assert np.array_equal(np.asarray(got, np.uint32), mixes["uniform"].astype(np.uint32))
        res[name] = round(statistics.median(ts), 1)
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
