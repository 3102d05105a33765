#!/usr/bin/env python3
"""The delivered packets of a routed batch packed for the copy back and the TUN write: what the pack costs on
the device, what it saves the incoming host pipeline, and what the packed TUN write costs the writing thread
(DESIGN.md 4.5 "Delivered packets packed on routed batches").

  pack      qgcm_deliver_pack of 2^20 packets in slots of 1536 bytes, hipEvent times of one call (its four
            kernels), warm, the median of --reps (at least 20), for three inputs -- 1354-byte packets all
            delivered, lengths uniform in 36..1444 with 10 % dropped, 64-byte packets -- with the bytes read and
            written per second beside the rate of qgcm_stream_copy (bench.py's copy_achievable) in the same run,
            and qgcm_gro_unpack and qgcm_chain_incoming of the same batch beside them
  pipeline  qgcm_route_chain_open_gro_host against qgcm_route_chain_open_gro_packed_host in one process,
            alternating, for 65536 and 2^20 sealed 1382-byte packets in 45-segment buffers, at stride 1536 and at
            stride 9216: wall milliseconds, the median of --pipeline-reps after a warm call, the existing call's
            own spread over its repeats, and the bytes up and down
  tun       thread-CPU microseconds per delivered packet of qgcm_tun_write_packed against qgcm_tun_write_slots
            called once per run of delivered slots (the host-side skip), on a TUN device where the host allows
            one; needs no GPU

Writes one JSON file per section into --out (default profiles/deliver_pack) and prints them.
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


def pack_section(reps):
    import torch

    from bench import GpuTelemetry, stream_copy_gbs
    from quantum_amd import route

    n, stride = 1 << 20, 1536
    ctx, addrs = make_ctx()
    rng = np.random.default_rng(0xDE11)

    def timed(fn, prep=None):
        def once():
            if prep:
                prep()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            return a.elapsed_time(b) * 1e3

        for _ in range(3):
            once()
        return round(statistics.median(once() for _ in range(reps)), 1)

    res = {"packets": n, "stride": stride, "reps": reps}
    tel = GpuTelemetry(0)
    tel.span = "the device timings"
    tel.start()
    res["copy_achievable_gb_s"] = round(stream_copy_gbs(ctx, 1 << 30, "cuda", torch.cuda.current_stream()), 1)

    # the batch: 1382-byte datagrams of known senders in 45-segment buffers, unpacked into the slots
    table, packed_len, total = packed_layout([(min(SEGS, n - k), DGRAM, DGRAM) for k in range(0, n, SEGS)])
    assert total == n
    packed_in = torch.randint(0, 256, ((packed_len + 15) & ~15,), dtype=torch.uint8, device="cuda")
    at = (torch.from_numpy(np.repeat(table[:, 0].astype(np.int64), SEGS)[:n]).cuda() +
          torch.arange(n, device="cuda") % SEGS * DGRAM)
    src = torch.from_numpy(addrs[rng.integers(0, PEERS, n)].view(np.uint8).reshape(n, 4).copy()).cuda()
    for k in range(4):
        packed_in[at + k] = src[:, k]
    d_bufs = torch.from_numpy(table.view(np.int32).reshape(-1).copy()).cuda()
    arena = torch.zeros(n * stride, dtype=torch.uint8, device="cuda")
    lens = torch.zeros(n, dtype=torch.int32, device="cuda")
    res["gro_unpack_us"] = timed(lambda: route.gro_unpack(ctx, packed_in, packed_len, d_bufs, len(table), n, arena, stride, lens))
    res["gro_unpack_gb_s"] = round(2 * int(table[:, 1].sum()) / (res["gro_unpack_us"] * 1e-6) / 1e9, 1)
    peer = torch.zeros(n, dtype=torch.int32, device="cuda")
    descs = torch.zeros(16 * n, dtype=torch.uint8, device="cuda")
    status = torch.zeros(n, dtype=torch.uint8, device="cuda")
    nbytes = torch.zeros(n, dtype=torch.int32, device="cuda")
    work = route.chain_work(n)
    dgram_lens = lens.clone()
    res["resolve_incoming_us"] = timed(lambda: route.resolve_incoming(ctx, arena, stride, n, lens, peer, descs))
    # random bytes: every tag fails, after the whole packet went through GHASH and CTR as a good one does; the
    # chain rewrites the lengths, so each call starts from the datagrams' and from a fresh resolve
    def fresh_resolve():
        lens.copy_(dgram_lens)
        route.resolve_incoming(ctx, arena, stride, n, lens, peer, descs)

    res["chain_incoming_us"] = timed(lambda: route.chain_incoming(ctx, arena, stride, n, lens, peer, descs,
                                                                  route.PLUGIN_ENCRYPTION, status, nbytes, work), fresh_resolve)
    del packed_in, d_bufs, descs, nbytes, work

    out = torch.zeros(n * stride, dtype=torch.uint8, device="cuda")
    recs = torch.zeros(4 * n, dtype=torch.int32, device="cuda")
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    pwork = route.deliver_pack_work(n)
    inputs = {"l1354_all_delivered": (np.full(n, 1354, np.uint32), np.ones(n, np.uint8)),
              "l36_1444_10pct_dropped": (rng.integers(36, 1445, n).astype(np.uint32), (rng.random(n) >= 0.1).astype(np.uint8)),
              "l64_all_delivered": (np.full(n, 64, np.uint32), np.ones(n, np.uint8))}
    for name, (h_lens, h_status) in inputs.items():
        lens.copy_(torch.from_numpy(h_lens.view(np.int32)))
        status.copy_(torch.from_numpy(h_status))
        us = timed(lambda: route.deliver_pack(ctx, arena, stride, n, lens, peer, status, out, n * stride, recs, counts, pwork))
        m, total = (int(v) for v in counts.cpu().numpy())
        ok = h_status == 1
        assert m == int(ok.sum()) and total == int(((4 + h_lens[ok].astype(np.int64) + 15) & ~15).sum())
        # read: the records' pieces, the lengths, statuses and peers (twice: the two scan passes read lens and
        # status), the table once by the copy; written: the records and the table
        moved = 2 * total + n * (2 * 5 + 4) + 2 * 16 * m
        res[f"{name}_pack_us"] = us
        res[f"{name}_records"] = m
        res[f"{name}_packed_bytes"] = total
        res[f"{name}_bytes_read_plus_written"] = moved
        res[f"{name}_gb_s"] = round(moved / (us * 1e-6) / 1e9, 1)
        res[f"{name}_share_of_copy_achievable"] = round(res[f"{name}_gb_s"] / res["copy_achievable_gb_s"], 3)
    tel.stop()
    res["sclk_mhz_mean"] = tel.summary().get("sclk_mhz_mean")
    ctx.close()
    return res


def pipeline_section(reps, sizes):
    from quantum_amd import _lib, route

    L = _lib.lib()
    ctx, addrs = make_ctx()
    base = 65536
    # one peer, and this node's own address routed to it: the datagrams carry it as their sender
    own = 10 | 99 << 8 | 1 << 24
    route.routes_set(ctx, {int(addrs[0]): 0, own: 0}, 10 | 99 << 8, 0xFFFF, 10 | 99 << 8 | 255 << 16 | 254 << 24, own)
    ptr, sealed, lens, _ = sealed_batch(ctx, addrs, base, np.zeros(base, np.int64))
    assert np.all(lens == DGRAM)
    res = {"bytes": DGRAM, "segments_per_buffer": SEGS, "reps": reps, "cpus": len(os.sched_getaffinity(0))}
    rec = (4 + TUN_LEN + 15) & ~15
    for n in sizes:
        table, packed_len, total = packed_layout([(min(SEGS, n - k), DGRAM, DGRAM) for k in range(0, n, SEGS)])
        assert total == n
        packed = np.zeros((packed_len + 15) & ~15, np.uint8)
        for off, length, _, first in table.tolist():  # the 65536 sealed datagrams, over and over
            idx = (first + np.arange(length // DGRAM)) % base
            packed[off:off + length] = sealed[idx, :DGRAM].reshape(-1)
        out_buf, recs = np.zeros(n * rec, np.uint8), np.zeros((n, 4), np.uint32)
        for stride in (1536, 9216):
            arena = np.zeros(n * stride, np.uint8)
            h_lens, peer, status = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint8)
            wall = {"slots_out": [], "packed_out": []}
            for rep in range(reps + 1):
                for which in ("slots_out", "packed_out"):
                    t0 = time.perf_counter()
                    if which == "slots_out":
                        dropped = route.route_chain_open_gro_host(ctx, packed, packed_len, table, arena.ctypes.data, stride,
                                                                  n, h_lens, route.PLUGIN_ENCRYPTION, peer, status)
                    else:
                        dropped, got, out = route.route_chain_open_gro_packed_host(ctx, packed, packed_len, table, stride, n,
                                                                                   h_lens, route.PLUGIN_ENCRYPTION, peer,
                                                                                   status, out_buf, recs)
                    t1 = time.perf_counter()
                    assert dropped == 0 and np.all(h_lens == TUN_LEN), (which, dropped)
                    if which == "packed_out":
                        assert out.tolist() == [n, n, n * rec] and int(got[-1, 0]) == (n - 1) * rec
                    if rep >= 1:  # one warm round
                        wall[which].append(t1 - t0)
            key = f"n{n}_stride{stride}"
            for which in ("slots_out", "packed_out"):
                res[f"{key}_{which}_ms"] = round(statistics.median(wall[which]) * 1e3, 2)
            res[f"{key}_slots_out_min_ms"] = round(min(wall["slots_out"]) * 1e3, 2)
            res[f"{key}_slots_out_max_ms"] = round(max(wall["slots_out"]) * 1e3, 2)
            res[f"{key}_packed_out_max_ms"] = round(max(wall["packed_out"]) * 1e3, 2)
            res[f"{key}_bytes_up"] = packed_len + 16 * len(table)
            res[f"{key}_bytes_down_slots_out"] = n * stride + 9 * n
            res[f"{key}_bytes_down_packed_out"] = n * rec + 16 * n + 9 * n
            res[f"{key}_ratio_slots_out_over_packed_out"] = round(res[f"{key}_slots_out_ms"] / res[f"{key}_packed_out_ms"], 2)
            print(json.dumps({k: v for k, v in res.items() if k.startswith(key)}), flush=True)
            del arena
    del sealed
    L.qgcm_host_free(ptr)
    ctx.close()
    return res


def tun_section(reps):
    import ctypes as C

    from quantum_amd import _lib, route
    from tests.test_tun_batch import HOST_IP, PEER_IP, _ipv4_udp

    L = _lib.lib()
    fds, name = (C.c_int * 1)(), C.create_string_buffer(16)
    rc = L.qgcm_tun_open(b"qgcmd%d", 1, fds, name, 16)
    if rc < 0:
        return {"measured": False, "why": f"TUN device refused (errno {-rc})"}
    try:
        rc = L.qgcm_tun_up(name.value, HOST_IP.encode(), 24, 1433)
        if rc < 0:
            return {"measured": False, "why": f"TUN link set-up refused (errno {-rc})"}
        n, stride = 65536, 1536
        rng = np.random.default_rng(0x7D1)
        # nobody listens on the port: the kernel takes every packet off the queue and drops it at the socket lookup
        pkt = np.frombuffer(_ipv4_udp(PEER_IP, HOST_IP, 7000, 9, os.urandom(1354 - 28)), np.uint8)
        arena = np.zeros((n, stride), np.uint8)
        arena[:, 4:4 + len(pkt)] = pkt
        lens, status = np.full(n, len(pkt), np.uint32), (rng.random(n) >= 0.1).astype(np.uint8)
        packed = np.zeros(n * 1360, np.uint8)
        recs, total = route.deliver_pack_cpu(arena.reshape(-1), stride, n, lens, np.zeros(n, np.uint32), status, packed)
        m = len(recs)
        # the host-side skip: one qgcm_tun_write_slots call per run of delivered slots
        edges = np.flatnonzero(np.diff(np.concatenate([[0], status, [0]]).astype(np.int8)))
        runs = list(zip(edges[0::2].tolist(), edges[1::2].tolist()))
        cpu = {"slots_with_skip": [], "packed": []}
        for rep in range(reps + 1):
            for which in ("slots_with_skip", "packed"):
                c0 = time.thread_time()
                if which == "packed":
                    wrote = route.tun_write_packed(fds[0], packed, total, recs)
                else:
                    wrote = 0
                    for a, b in runs:
                        wrote += L.qgcm_tun_write_slots(fds[0], arena.ctypes.data + a * stride, stride, b - a, lens.ctypes.data + 4 * a)
                c1 = time.thread_time()
                assert wrote == m, (which, wrote, m)
                if rep >= 1:
                    cpu[which].append(c1 - c0)
        res = {"measured": True, "packets": n, "delivered": m, "packet_bytes": int(len(pkt)), "runs_of_delivered_slots": len(runs),
               "reps": reps}
        for which in cpu:
            res[f"{which}_cpu_us_per_delivered_packet"] = round(statistics.median(cpu[which]) / m * 1e6, 4)
        # what of the skip loop is this script's own: the same calls with nothing to write
        c0 = time.thread_time()
        for a, b in runs:
            L.qgcm_tun_write_slots(fds[0], arena.ctypes.data + a * stride, stride, 0, lens.ctypes.data + 4 * a)
        res["skip_loop_empty_calls_cpu_us_per_delivered_packet"] = round((time.thread_time() - c0) / m * 1e6, 4)
        return res
    finally:
        L.qgcm_tun_close(fds[0])


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--pipeline-reps", type=int, default=3)
    ap.add_argument("--pipeline-sizes", default="65536,1048576")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deliver_pack"))
    ap.add_argument("--sections", default="pack,pipeline,tun")
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    run = {"pack": lambda: pack_section(max(20, args.reps)),
           "pipeline": lambda: pipeline_section(max(1, args.pipeline_reps), [int(s) for s in args.pipeline_sizes.split(",")]),
           "tun": lambda: tun_section(5)}
    for name in args.sections.split(","):
        res = run[name]()
        with open(os.path.join(args.out, f"{name}.json"), "w") as f:
            f.write(json.dumps(res) + "\n")
        print(json.dumps({name: res}), flush=True)


if __name__ == "__main__":
    main()
