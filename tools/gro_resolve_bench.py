#!/usr/bin/env python3
"""Coalesced receive buffers unpacked into slots and resolved in one launch: what the fused kernel costs beside
the pair of launches it replaces, and what it does to the incoming host pipeline (DESIGN.md 4.5 "Coalesced buffers
unpacked and resolved in one launch").

  device    qgcm_gro_resolve of 2^20 datagrams from 1 024 keyed senders into slots of 1536 bytes against the pair
            qgcm_gro_unpack + qgcm_resolve_incoming: hipEvent times, warm, in alternating rounds, the median of
            --reps (at least 20) and each form's fastest and slowest round, for the three mixes of
            tools/gro_recv_bench.py -- 1382-byte datagrams in 45-segment buffers, lengths uniform in 64..1472 in
            buffers of 1..64 segments, lone 64-byte datagrams -- with the unpack and the resolve timed alone, the
            bytes read and written per second beside the rate of qgcm_stream_copy in the same run, and the mean
            clock.  Before the timing both forms run over the same sentinel-filled memory and their outputs are
            compared whole.
  pipeline  qgcm_route_chain_open_gro_packed_host on a context created under QGCM_GRO_FUSED=0 (the pair) against
            one created under QGCM_GRO_FUSED=1 (the one launch), alternating in one process, for 65536 and 2^20
            sealed 1382-byte packets in 45-segment buffers at stride 1536: wall milliseconds, the median of
            --pipeline-reps after a warm round, with each form's fastest and slowest round

Writes one JSON file per section into --out (default profiles/gro_resolve) and prints them.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.gro_recv_bench import DGRAM, SEGS, packed_layout, sealed_batch  # noqa: E402
from tools.send_plan_bench import PEERS, TUN_LEN, make_ctx  # noqa: E402


def shapes_of(n, rng):
    shapes = {"d1382_in_45_segment_buffers": [(min(SEGS, n - k), DGRAM, DGRAM) for k in range(0, n, SEGS)]}
    mixed, left = [], n
    while left:
        c = int(min(rng.integers(1, 65), left))
        seg = int(rng.integers(64, min(1472, 65535 // c) + 1))
        mixed.append((c, seg, int(rng.integers(1, seg + 1))))
        left -= c
    shapes["lengths_64_1472_in_mixed_buffers"] = mixed
    shapes["lone_64_byte_datagrams"] = [(1, 64, 64)] * n
    return shapes


def sources_of(table, n):
    """The packed offset of every datagram of an ascending, gapless table, whole arrays at a time."""
    length, seg = table[:, 1].astype(np.int64), table[:, 2].astype(np.int64)
    count = np.where((seg == 0) | (seg >= length), 1, -(-length // np.maximum(seg, 1)))
    assert int(count.sum()) == n
    which = np.repeat(np.arange(len(table)), count)
    k = np.arange(n) - table[which, 3].astype(np.int64)
    src = table[which, 0].astype(np.int64) + k * seg[which]
    left = length[which] - k * seg[which]
    return src, np.where(count[which] == 1, length[which], np.minimum(left, seg[which]))


def device_section(reps):
    import torch

    from bench import GpuTelemetry, stream_copy_gbs
    from quantum_amd import route

    n, stride = 1 << 20, 1536
    ctx, addrs = make_ctx()
    rng = np.random.default_rng(0x6A11)

    def once(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3

    def alternating(fns):
        """`reps` timings of each, taken in alternating rounds after three warm ones."""
        took = {k: [] for k in fns}
        for rep in range(reps + 3):
            for k, fn in fns.items():
                us = once(fn)
                if rep >= 3:
                    took[k].append(us)
        return took

    res = {"datagrams": n, "stride": stride, "max_keys": PEERS, "reps": reps}
    tel = GpuTelemetry(0)
    tel.span = "the device timings"
    tel.start()
    res["copy_achievable_gb_s"] = round(stream_copy_gbs(ctx, 1 << 30, "cuda", torch.cuda.current_stream()), 1)
    outs = [dict(arena=torch.empty(n * stride, dtype=torch.uint8, device="cuda"), lens=torch.empty(n, dtype=torch.int32, device="cuda"),
                 peer=torch.empty(n, dtype=torch.int32, device="cuda"), descs=torch.empty(16 * n, dtype=torch.uint8, device="cuda"))
            for _ in range(2)]
    for name, shape in shapes_of(n, rng).items():
        table, packed_len, total = packed_layout(shape)
        assert total == n
        packed = torch.randint(0, 256, ((packed_len + 15) & ~15,), dtype=torch.uint8, device="cuda")
        src, dlen = sources_of(table, n)
        named = np.flatnonzero(dlen >= 4)
        at = torch.from_numpy(src[named]).cuda()[:, None] + torch.arange(4, device="cuda")[None, :]
        sender = torch.from_numpy(addrs[rng.integers(0, PEERS, len(named))].view(np.uint8).reshape(-1, 4).copy()).cuda()
        packed[at.reshape(-1)] = sender.reshape(-1)  # Raw[0:4]: senders the route table knows
        del at, sender
        d_bufs = torch.from_numpy(table.view(np.int32).reshape(-1).copy()).cuda()
        nb = len(table)

        def fused(o=outs[0]):
            route.gro_resolve(ctx, packed, packed_len, d_bufs, nb, n, o["arena"], stride, o["lens"], o["peer"], o["descs"])

        def unpack(o=outs[1]):
            route.gro_unpack(ctx, packed, packed_len, d_bufs, nb, n, o["arena"], stride, o["lens"])

        def resolve(o=outs[1]):
            route.resolve_incoming(ctx, o["arena"], stride, n, o["lens"], o["peer"], o["descs"])

        def pair():
            unpack()
            resolve()

        # both forms over the same sentinel-filled memory: identical outputs, whole
        for o in outs:
            o["arena"].fill_(0xA5)
            o["lens"].fill_(0x5A5A5A5A)
            o["peer"].fill_(0x0BADF00D)
            o["descs"].fill_(0xA5)
        fused()
        pair()
        torch.cuda.synchronize()
        for k in outs[0]:
            assert torch.equal(outs[0][k], outs[1][k]), (name, k)
        hits = int((outs[0]["peer"] != -1).sum())
        assert hits == len(named), (name, hits, len(named))

        took = alternating({"fused": fused, "pair": pair, "unpack": unpack, "resolve": resolve})
        med = {k: round(statistics.median(v), 1) for k, v in took.items()}
        total_bytes = int(table[:, 1].sum())
        # read: the datagrams' bytes, the table, one route entry a datagram; written: the datagrams' bytes, lens,
        # peer, descs
        moved = 2 * total_bytes + 16 * nb + 8 * n + 4 * n + 4 * n + 16 * n
        res[f"{name}_buffers"] = nb
        res[f"{name}_gro_resolve_us"] = med["fused"]
        res[f"{name}_gro_resolve_min_us"] = round(min(took["fused"]), 1)
        res[f"{name}_gro_resolve_max_us"] = round(max(took["fused"]), 1)
        res[f"{name}_pair_us"] = med["pair"]
        res[f"{name}_pair_min_us"] = round(min(took["pair"]), 1)
        res[f"{name}_pair_max_us"] = round(max(took["pair"]), 1)
        res[f"{name}_gro_unpack_us"] = med["unpack"]
        res[f"{name}_resolve_incoming_us"] = med["resolve"]
        res[f"{name}_pair_over_fused"] = round(med["pair"] / med["fused"], 2)
        res[f"{name}_fused_median_at_or_below_pair_median"] = med["fused"] <= med["pair"]
        res[f"{name}_fused_median_below_pair_min"] = med["fused"] < min(took["pair"])
        res[f"{name}_bytes_read_plus_written"] = moved
        res[f"{name}_gb_s"] = round(moved / (med["fused"] * 1e-6) / 1e9, 1)
        res[f"{name}_pair_gb_s"] = round(moved / (med["pair"] * 1e-6) / 1e9, 1)
        res[f"{name}_share_of_copy_achievable"] = round(res[f"{name}_gb_s"] / res["copy_achievable_gb_s"], 3)
        print(json.dumps({k: v for k, v in res.items() if k.startswith(name)}), flush=True)
        del packed, d_bufs
    tel.stop()
    res["sclk_mhz_mean"] = tel.summary().get("sclk_mhz_mean")
    res["fused_at_or_below_pair_on_every_mix"] = all(v for k, v in res.items() if k.endswith("_fused_median_at_or_below_pair_median"))
    ctx.close()
    return res


def pipeline_section(reps, sizes):
    from quantum_amd import _lib, route

    L = _lib.lib()
    ctxs = {"pair": make_ctx(QGCM_GRO_FUSED=0), "fused": make_ctx(QGCM_GRO_FUSED=1)}
    addrs = ctxs["pair"][1]
    base, stride = 65536, 1536
    # one peer, and this node's own address routed to it: the datagrams carry it as their sender
    own = 10 | 99 << 8 | 1 << 24
    for ctx, _ in ctxs.values():
        route.routes_set(ctx, {int(addrs[0]): 0, own: 0}, 10 | 99 << 8, 0xFFFF, 10 | 99 << 8 | 255 << 16 | 254 << 24, own)
    ptr, sealed, lens, _ = sealed_batch(ctxs["pair"][0], addrs, base, np.zeros(base, np.int64))
    assert np.all(lens == DGRAM)
    res = {"bytes": DGRAM, "segments_per_buffer": SEGS, "stride": stride, "reps": reps, "cpus": len(os.sched_getaffinity(0))}
    for n in sizes:
        table, packed_len, total = packed_layout([(min(SEGS, n - k), DGRAM, DGRAM) for k in range(0, n, SEGS)])
        assert total == n
        packed = np.zeros((packed_len + 15) & ~15, np.uint8)
        for off, length, _, first in table.tolist():  # the 65536 sealed datagrams, over and over
            idx = (first + np.arange(length // DGRAM)) % base
            packed[off:off + length] = sealed[idx, :DGRAM].reshape(-1)
        out_buf, recs = np.zeros(n * ((4 + TUN_LEN + 15) & ~15), np.uint8), np.zeros((n, 4), np.uint32)
        h_lens, peer, status = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint8)
        wall = {k: [] for k in ctxs}
        for rep in range(reps + 1):
            for which, (ctx, _) in ctxs.items():
                t0 = time.perf_counter()
                dropped, _, out = route.route_chain_open_gro_packed_host(ctx, packed, packed_len, table, stride, n, h_lens,
                                                                         route.PLUGIN_ENCRYPTION, peer, status, out_buf, recs)
                t1 = time.perf_counter()
                assert dropped == 0 and int(out[0]) == n and int(out[1]) == n and np.all(h_lens == TUN_LEN), (which, dropped)
                if rep >= 1:  # one warm round
                    wall[which].append(t1 - t0)
        key = f"n{n}"
        for which in ctxs:
            res[f"{key}_{which}_ms"] = round(statistics.median(wall[which]) * 1e3, 2)
            res[f"{key}_{which}_min_ms"] = round(min(wall[which]) * 1e3, 2)
            res[f"{key}_{which}_max_ms"] = round(max(wall[which]) * 1e3, 2)
        res[f"{key}_ratio_pair_over_fused"] = round(res[f"{key}_pair_ms"] / res[f"{key}_fused_ms"], 3)
        res[f"{key}_fused_median_at_or_below_pair_max"] = res[f"{key}_fused_ms"] <= res[f"{key}_pair_max_ms"]
        print(json.dumps({k: v for k, v in res.items() if k.startswith(key)}), flush=True)
        del packed, out_buf
    del sealed
    L.qgcm_host_free(ptr)
    for ctx, _ in ctxs.values():
        ctx.close()
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--pipeline-reps", type=int, default=3)
    ap.add_argument("--pipeline-sizes", default="65536,1048576")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gro_resolve"))
    ap.add_argument("--sections", default="device,pipeline")
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    run = {"device": lambda: device_section(max(20, args.reps)),
           "pipeline": lambda: pipeline_section(max(1, args.pipeline_reps), [int(s) for s in args.pipeline_sizes.split(",")])}
    for name in args.sections.split(","):
        res = run[name]()
        with open(os.path.join(args.out, f"{name}.json"), "w") as f:
            f.write(json.dumps(res) + "\n")
        print(json.dumps({name: res}), flush=True)


if __name__ == "__main__":
    main()
