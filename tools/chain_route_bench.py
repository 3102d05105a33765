#!/usr/bin/env python3
"""The plugin chain on a routed batch beside the existing launches that do the same work.

2^20 slots of stride 1472 holding the 1350-byte config-5 packet (quantum_amd/workloads.py), 1024 peers,
device-resident.  Three flag mixes: every peer both plugins ("both"); a quarter of the peers each combination
("quarter"); encryption only ("enc").  Per mix, hipEvent times of one call, warm, the median of --reps
repetitions (at least 20) -- the chain works in place, so every repetition starts from a device copy of the
batch made outside the timed span:
  * qgcm_chain_outgoing and qgcm_chain_incoming (the incoming batch is what the peers would send: the outgoing
    result sealed under each peer's own address as additional data),
  * the comparator, existing launches in the same process on the same packets with per-peer descriptors:
    "both": qgcm_snappy_compress_batch + qgcm_seal_batch, and qgcm_open_batch + qgcm_snappy_uncompress_batch;
    "enc": qgcm_seal_batch / qgcm_open_batch alone.  "quarter" has none: no existing launch gates per peer.
  * the elementwise kernels alone: the chain with plugins = 0 (outgoing: plan + finish; incoming: the fused mid).
Prints one JSON line with the GPU's mean clock over the device timings.  The point of comparison for the glue is
the resolve launch of the same batch (tools/route_bench.py), timed here as well.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=1 << 20)
    ap.add_argument("--peers", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    reps = max(20, args.reps)
    import torch

    from quantum_amd import batch, route, workloads
    from quantum_amd.crypto import Context

    n, peers, stride, L = args.slots, args.peers, workloads.C5_STRIDE, workloads.C5_LEN
    rng = np.random.default_rng(0xC4A1B)
    ctx = Context(device=0, max_keys=peers)
    ctx.set_keys(0, rng.integers(0, 256, 32 * peers, dtype=np.uint8).tobytes())
    addrs = np.array([10 | 99 << 8 | (j >> 8) << 16 | (j & 255) << 24 for j in range(2, 2 + peers)], np.uint32)
    net, mask, own = 10 | 99 << 8, 0xFFFF, 10 | 99 << 8 | 1 << 24
    route.routes_set(ctx, {int(a): k for k, a in enumerate(addrs)}, net, mask, 10 | 99 << 8 | 255 << 16 | 254 << 24, own)
    # the config-5 packet, 4096 distinct ones tiled (the host generator makes 2^20 in minutes)
    tile = workloads.config5_packets(4096, L, stride)
    dest = rng.integers(0, peers, n)
    pristine = torch.from_numpy(tile).cuda().repeat(n // 4096 + 1, 1)[:n].contiguous()
    pristine[:, 20:24] = torch.from_numpy(addrs[dest].view(np.uint8).reshape(n, 4).copy()).cuda()
    sender = torch.from_numpy(addrs[dest].view(np.uint8).reshape(n, 4).copy()).cuda()
    arena = torch.empty_like(pristine)
    lens0 = torch.full((n,), L, dtype=torch.int32, device="cuda")
    lens = lens0.clone()
    peer = torch.zeros(n, dtype=torch.int32, device="cuda")
    descs = torch.zeros(16 * n, dtype=torch.uint8, device="cuda")
    status = torch.zeros(n, dtype=torch.uint8, device="cuda")
    nbytes = torch.zeros(n, dtype=torch.int32, device="cuda")
    work = route.chain_work(n)
    d_peer = torch.from_numpy(dest.astype(np.int32)).cuda()
    offs = np.arange(n, dtype=np.uint64) * stride

    def timed(fn, src, src_lens):
        def once():
            arena.copy_(src)
            lens.copy_(src_lens)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            return a.elapsed_time(b) * 1e3

        for _ in range(3):
            once()
        return round(statistics.median(once() for _ in range(reps)), 1)

    res = {"slots": n, "stride": stride, "len": L, "peers": peers, "reps": reps}
    from bench import GpuTelemetry  # the box's clock over the device timings, as bench.py reports it

    tel = GpuTelemetry(0)
    tel.span = "the device timings"
    tel.start()
    res["resolve_outgoing_us"] = timed(lambda: route.resolve_outgoing(ctx, arena, stride, n, lens, peer, descs), pristine, lens0)
    resolved = arena.clone()  # own_ip written; the peers' own addresses as additional data for the way back in
    as_peers = resolved.clone()
    as_peers[:, 0:4] = sender
    mixes = {"both": np.full(peers, 3, np.uint8), "quarter": (np.arange(peers) % 4).astype(np.uint8),
             "enc": np.full(peers, 2, np.uint8)}
    for mix, flags in mixes.items():
        route.peer_plugins_set(ctx, 0, flags.tobytes())
        out = lambda: route.chain_outgoing(ctx, arena, stride, n, lens, d_peer, descs, 3, None, status, nbytes, work)
        res[f"{mix}_chain_outgoing_us"] = timed(out, resolved, lens0)
        assert int(status.sum()) == n, f"{mix}: outgoing dropped packets"
        timed(out, as_peers, lens0)  # the same batch as the peers send it
        grams, m = arena.clone(), lens.clone()
        route.resolve_incoming(ctx, grams, stride, n, m, peer, descs)
        torch.cuda.synchronize()
        assert np.array_equal(peer.cpu().numpy(), dest.astype(np.int32)), "incoming resolve is wrong"
        res[f"{mix}_chain_incoming_us"] = timed(
            lambda: route.chain_incoming(ctx, arena, stride, n, lens, d_peer, descs, 3, status, nbytes, work), grams, m)
        assert int(status.sum()) == n and bool((lens == L).all()), f"{mix}: incoming did not restore the packets"
        assert bool((arena[:, 4:4 + L] == pristine[:, 4:4 + L]).all()), f"{mix}: incoming bytes differ"
        if mix == "quarter":
            continue
        # the comparators: existing launches, per-peer descriptors made outside the timed span
        clen = (m.cpu().numpy().astype(np.int64) - 32)  # the packet each datagram carries, compressed or not
        seal_descs = batch.make_descs(offs, clen, dest, "cuda")
        open_descs = batch.make_descs(offs, clen + 28, dest, "cuda")
        clens = torch.from_numpy(clen.astype(np.int32)).cuda()
        if mix == "both":
            def seal_side():
                batch.snappy_compress(ctx, arena, stride, n, lens, stride - 4, stride - 32, status)
                batch.seal_batch(ctx, arena, seal_descs, n, None, status=status)

            def open_side():
                batch.open_batch(ctx, arena, open_descs, n, status=status)
                batch.snappy_uncompress(ctx, arena, stride, n, lens, stride - 4, stride - 4, status)

            res["both_compress_seal_us"] = timed(seal_side, resolved, lens0)
            res["both_open_uncompress_us"] = timed(open_side, grams, clens)
            assert int(status.sum()) == n and bool((arena[:, 4:4 + L] == pristine[:, 4:4 + L]).all())
        else:
            res["enc_seal_batch_us"] = timed(lambda: batch.seal_batch(ctx, arena, seal_descs, n, None, status=status), resolved, lens0)
            res["enc_open_batch_us"] = timed(lambda: batch.open_batch(ctx, arena, open_descs, n, status=status), grams, m)
            assert int(status.sum()) == n
    # the elementwise kernels alone
    res["glue_outgoing_plan_finish_us"] = timed(
        lambda: route.chain_outgoing(ctx, arena, stride, n, lens, d_peer, descs, 0, None, status, nbytes, work), resolved, lens0)
    res["glue_incoming_mid_us"] = timed(
        lambda: route.chain_incoming(ctx, arena, stride, n, lens, d_peer, descs, 0, status, nbytes, work), resolved, lens0)
    res["account_bytes_us"] = timed(lambda: route.route_account_bytes(ctx, route.TX, n, d_peer, nbytes, status), resolved, lens0)
    tel.stop()
    res["sclk_mhz_mean"] = tel.summary().get("sclk_mhz_mean")
    for mix in ("both", "enc"):
        a, b = ("compress_seal", "open_uncompress") if mix == "both" else ("seal_batch", "open_batch")
        res[f"{mix}_outgoing_excess_us"] = round(res[f"{mix}_chain_outgoing_us"] - res[f"{mix}_{a}_us"], 1)
        res[f"{mix}_incoming_excess_us"] = round(res[f"{mix}_chain_incoming_us"] - res[f"{mix}_{b}_us"], 1)
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
