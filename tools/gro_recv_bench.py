#!/usr/bin/env python3
"""The coalesced receive of a routed batch: what the unpack costs on the device, what the coalesced receive
saves the receiving thread on a loopback socket, and what the packed copy-in saves the incoming host pipeline
(DESIGN.md 4.5 "Coalesced receive on routed batches").

  unpack    qgcm_gro_unpack of 2^20 datagrams into slots of 1536 bytes, hipEvent times of one call, warm, the
            median of --reps (at least 20), for three mixes -- 1382-byte datagrams in 45-segment buffers,
            lengths uniform in 64..1472 in buffers of 1..64 segments, lone 64-byte datagrams -- with the bytes
            read and written per second beside the rate of qgcm_stream_copy (bench.py's copy_achievable), and
            qgcm_resolve_incoming and qgcm_open_batch of the first mix's batch beside them
  receive   16384 sealed 1382-byte datagrams sent with qgcm_udp_send_plan to one loopback socket in windows the
            socket buffer holds, received by a thread of its own with qgcm_udp_recv_slots and with
            qgcm_udp_recv_gro (UDP_GRO on), alternating in one process: thread-CPU microseconds per datagram,
            the median of 10, for one peer, 16 peers round-robin and 1024 peers uniform; the share of buffers
            that arrived coalesced and the datagrams per buffer
  pipeline  qgcm_route_chain_open_host (its arena already slotted) against qgcm_route_chain_open_gro_host (the
            packed area and its table) for 65536 and 2^20 sealed 1382-byte packets in 45-segment buffers, at
            stride 1536 and at stride 9216: wall milliseconds, the median of --pipeline-reps

Writes one JSON file per section into --out (default profiles/gro_recv) and prints them.
"""
from __future__ import annotations

import argparse
import json
import os
import platform
import socket
import statistics
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.send_plan_bench import PEERS, STRIDE, TUN_LEN, make_ctx  # noqa: E402

DGRAM = TUN_LEN + 32  # 1382
SEGS = 45             # 45 * 1382 = 62190 bytes: the longest train of that length under 65507


def packed_layout(lengths_per_buffer):
    """Buffers back to back at 16-B-aligned offsets, as qgcm_udp_recv_gro leaves them: per buffer (count, seg,
    last) -> (table (n_bufs, 4) uint32, packed_len, n)."""
    bufs, at, first = [], 0, 0
    for count, seg, last in lengths_per_buffer:
        length = (count - 1) * seg + last
        bufs.append((at, length, seg if count > 1 else 0, first))
        first += count
        at = (at + length + 15) & ~15
    table = np.array(bufs, np.uint32).reshape(-1, 4)
    return table, int(table[-1, 0]) + int(table[-1, 1]), first


def unpack_section(reps):
    import torch

    from bench import GpuTelemetry, stream_copy_gbs
    from quantum_amd import batch, route

    n, stride = 1 << 20, 1536
    ctx, addrs = make_ctx()
    rng = np.random.default_rng(0x6A01)
    shapes = {"d1382_in_45_segment_buffers": [(min(SEGS, n - k), DGRAM, DGRAM) for k in range(0, n, SEGS)],
              "lone_64_byte_datagrams": [(1, 64, 64)] * n}
    mixed, left = [], n
    while left:
        c = int(min(rng.integers(1, 65), left))
        seg = int(rng.integers(64, min(1472, 65535 // c) + 1))
        mixed.append((c, seg, int(rng.integers(1, seg + 1))))
        left -= c
    shapes["lengths_64_1472_in_mixed_buffers"] = mixed

    def timed(fn):
        def once():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            return a.elapsed_time(b) * 1e3

        for _ in range(3):
            once()
        return round(statistics.median(once() for _ in range(reps)), 1)

    res = {"datagrams": n, "stride": stride, "reps": reps}
    arena = torch.zeros(n * stride, dtype=torch.uint8, device="cuda")
    lens = torch.zeros(n, dtype=torch.int32, device="cuda")
    tel = GpuTelemetry(0)
    tel.span = "the device timings"
    tel.start()
    res["copy_achievable_gb_s"] = round(stream_copy_gbs(ctx, 1 << 30, "cuda", torch.cuda.current_stream()), 1)
    for name in ("d1382_in_45_segment_buffers", "lengths_64_1472_in_mixed_buffers", "lone_64_byte_datagrams"):
        table, packed_len, total = packed_layout(shapes[name])
        assert total == n
        packed = torch.randint(0, 256, ((packed_len + 15) & ~15,), dtype=torch.uint8, device="cuda")
        if name.startswith("d1382"):
            # senders the route table knows, so that the resolve and the open beside it have work to do
            at = (torch.from_numpy(np.repeat(table[:, 0].astype(np.int64), SEGS)[:n]).cuda() +
                  torch.arange(n, device="cuda") % SEGS * DGRAM)
            src = torch.from_numpy(addrs[rng.integers(0, PEERS, n)].view(np.uint8).reshape(n, 4).copy()).cuda()
            for k in range(4):
                packed[at + k] = src[:, k]
        d_bufs = torch.from_numpy(table.view(np.int32).reshape(-1).copy()).cuda()
        us = timed(lambda: route.gro_unpack(ctx, packed, packed_len, d_bufs, len(table), n, arena, stride, lens))
        moved = 2 * int(table[:, 1].sum())  # every datagram byte read once and written once
        res[f"{name}_unpack_us"] = us
        res[f"{name}_buffers"] = int(len(table))
        res[f"{name}_bytes_read_plus_written"] = moved
        res[f"{name}_gb_s"] = round(moved / (us * 1e-6) / 1e9, 1)
        if name.startswith("d1382"):
            peer = torch.zeros(n, dtype=torch.int32, device="cuda")
            descs = torch.zeros(16 * n, dtype=torch.uint8, device="cuda")
            status = torch.zeros(n, dtype=torch.uint8, device="cuda")
            res["resolve_incoming_us"] = timed(lambda: route.resolve_incoming(ctx, arena, stride, n, lens, peer, descs))
            # random bytes: every tag fails, after the whole packet went through GHASH and CTR as a good one does
            res["open_batch_us"] = timed(lambda: batch.open_batch(ctx, arena, descs, n, status=status))
        del packed, d_bufs
    tel.stop()
    res["sclk_mhz_mean"] = tel.summary().get("sclk_mhz_mean")
    ctx.close()
    return res


def sealed_batch(ctx, addrs, n, dest):
    """n sealed 1382-byte datagrams in slots of 1472 bytes (pinned), their lengths and peers."""
    import ctypes as C

    from quantum_amd import _lib, batch, route

    rng = np.random.default_rng(0x5EA1 + n)
    ptr = _lib.lib().qgcm_host_alloc(n * STRIDE)
    assert ptr
    arena = np.frombuffer((C.c_uint8 * (n * STRIDE)).from_address(ptr), np.uint8).reshape(n, STRIDE)
    arena[:] = rng.integers(0, 256, (n, STRIDE), dtype=np.uint8)
    arena[:, 20:24] = addrs[dest].view(np.uint8).reshape(n, 4)
    lens, peer = np.full(n, TUN_LEN, np.uint32), np.zeros(n, np.uint32)
    assert route.route_chain_seal_host(ctx, ptr, STRIDE, n, lens, batch.GENERATE, route.PLUGIN_ENCRYPTION, peer) == 0
    return ptr, arena, lens, peer


def receive_section(reps):
    from quantum_amd import _lib, route

    L = _lib.lib()
    n = 16384
    ctx, addrs = make_ctx()
    rng = np.random.default_rng(0x5E2D)
    rx, tx = L.qgcm_udp_socket(b"127.0.0.1", 0, 1 << 22), L.qgcm_udp_socket(b"127.0.0.1", 0, 1 << 22)
    assert rx >= 0 and tx >= 0
    probe = socket.socket(fileno=os.dup(rx))
    rcvbuf = probe.getsockopt(socket.SOL_SOCKET, socket.SO_RCVBUF)
    probe.close()
    # a window the socket buffer holds whatever each datagram's buffer is charged (at most 4608 bytes here)
    window = int(max(64, min(4096, rcvbuf // 4608)))
    peer_addrs = route.peer_addrs([("127.0.0.1", L.qgcm_udp_port(rx))] * PEERS)
    res = {"datagrams": n, "bytes": DGRAM, "reps": reps, "kernel": platform.release(), "so_rcvbuf": rcvbuf,
           "window_datagrams": window}
    dests = {"one_peer": np.zeros(n, np.int64), "peers16_round_robin": np.arange(n) % 16,
             "peers1024_uniform": rng.integers(0, PEERS, n)}
    slots_buf, slots_len = np.zeros((4096 + 64, STRIDE), np.uint8), np.zeros(4096 + 64, np.uint32)
    packed, table, out = np.zeros(8 << 20, np.uint8), np.zeros((4096 + 64, 4), np.uint32), np.zeros(3, np.uint64)
    for name, dest in dests.items():
        ptr, arena, lens, peer = sealed_batch(ctx, addrs, n, dest)
        order, trains = route.send_plan_host(ctx, lens, peer)
        groups, a, held = [], 0, 0  # whole trains per window
        for t in range(len(trains)):
            if held + int(trains[t, 1]) > window:
                groups.append((a, t, held))
                a, held = t, 0
            held += int(trains[t, 1])
        groups.append((a, len(trains), held))
        cpu = {"slots": [], "gro": []}
        seen = {"buffers": 0, "coalesced": 0, "datagrams": 0}
        for rep in range(reps + 2):
            for which in ("slots", "gro"):
                route.udp_gro(rx, which == "gro")
                got, spent, want = [0], [0.0], [0]
                go, done = threading.Semaphore(0), threading.Semaphore(0)

                def receiver():
                    for _ in groups:
                        go.acquire()
                        c0 = time.thread_time()
                        while got[0] < want[0]:
                            if which == "gro":
                                r = route.udp_recv_gro(rx, packed, table, 4096 + 64, 1000, out)
                                if rep == 1 and r > 0:  # counted in a warm round, outside the timed ones
                                    seen["buffers"] += int(out[0])
                                    seen["coalesced"] += int(np.count_nonzero(table[:int(out[0]), 2]))
                                    seen["datagrams"] += r
                            else:
                                r = L.qgcm_udp_recv_slots(rx, slots_buf.ctypes.data, STRIDE, 4096 + 64, slots_len.ctypes.data, 1000)
                            assert r > 0, (which, r, got[0], want[0])
                            got[0] += r
                        spent[0] += time.thread_time() - c0
                        done.release()

                th = threading.Thread(target=receiver)
                th.start()
                for a, b, held in groups:
                    sent = route.udp_send_plan(tx, ptr, STRIDE, n, lens, order, trains[a:b], peer_addrs, PEERS)
                    assert sent == held, (sent, held)
                    want[0] += held
                    go.release()
                    done.acquire()
                th.join()
                assert got[0] == n
                if rep >= 2:  # two warm rounds
                    cpu[which].append(spent[0])
        for which in ("slots", "gro"):
            res[f"{name}_recv_{which}_cpu_us_per_datagram"] = round(statistics.median(cpu[which]) / n * 1e6, 4)
        res[f"{name}_trains"] = int(len(trains))
        res[f"{name}_coalesced_share_of_buffers"] = round(seen["coalesced"] / max(1, seen["buffers"]), 4)
        res[f"{name}_datagrams_per_buffer"] = round(seen["datagrams"] / max(1, seen["buffers"]), 2)
        res[f"{name}_cpu_ratio_slots_over_gro"] = round(res[f"{name}_recv_slots_cpu_us_per_datagram"] /
                                                      res[f"{name}_recv_gro_cpu_us_per_datagram"], 2)
        del arena
        L.qgcm_host_free(ptr)
    for fd in (rx, tx):
        L.qgcm_udp_close(fd)
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
    for n in sizes:
        table, packed_len, total = packed_layout([(min(SEGS, n - k), DGRAM, DGRAM) for k in range(0, n, SEGS)])
        assert total == n
        packed = np.zeros((packed_len + 15) & ~15, np.uint8)
        for b, (off, length, _, first) in enumerate(table.tolist()):  # the 65536 sealed datagrams, over and over
            c = length // DGRAM
            idx = (first + np.arange(c)) % base
            packed[off:off + length] = sealed[idx, :DGRAM].reshape(-1)
        for stride in (1536, 9216):
            arena = np.zeros(n * stride, np.uint8)
            h_lens, peer, status = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint8)
            wall = {"slots": [], "gro": []}
            for rep in range(reps + 1):
                for which in ("slots", "gro"):
                    if which == "slots":  # what qgcm_udp_recv_slots would have left: not timed
                        route.gro_unpack_cpu(packed, packed_len, table, n, arena, stride, h_lens)
                    t0 = time.perf_counter()
                    if which == "slots":
                        dropped = route.route_chain_open_host(ctx, arena.ctypes.data, stride, n, h_lens,
                                                              route.PLUGIN_ENCRYPTION, peer, status)
                    else:
                        dropped = route.route_chain_open_gro_host(ctx, packed, packed_len, table, arena.ctypes.data, stride,
                                                                  n, h_lens, route.PLUGIN_ENCRYPTION, peer, status)
                    t1 = time.perf_counter()
                    assert dropped == 0 and np.all(h_lens == TUN_LEN), (which, dropped)
                    if rep >= 1:  # one warm round
                        wall[which].append(t1 - t0)
            for which in ("slots", "gro"):
                res[f"n{n}_stride{stride}_{which}_ms"] = round(statistics.median(wall[which]) * 1e3, 2)
            res[f"n{n}_stride{stride}_bytes_up_slots"] = n * stride
            res[f"n{n}_stride{stride}_bytes_up_gro"] = packed_len + 16 * len(table)
            res[f"n{n}_stride{stride}_ratio_slots_over_gro"] = round(res[f"n{n}_stride{stride}_slots_ms"] /
                                                                    res[f"n{n}_stride{stride}_gro_ms"], 2)
            print(json.dumps({k: v for k, v in res.items() if k.startswith(f"n{n}_stride{stride}")}), flush=True)
            del arena
    del sealed
    L.qgcm_host_free(ptr)
    ctx.close()
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--pipeline-reps", type=int, default=3)
    ap.add_argument("--pipeline-sizes", default="65536,1048576")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gro_recv"))
    ap.add_argument("--sections", default="unpack,receive,pipeline")
    args = ap.parse_args()
    reps = max(20, args.reps)
    os.makedirs(args.out, exist_ok=True)
    run = {"unpack": lambda: unpack_section(reps), "receive": lambda: receive_section(10),
           "pipeline": lambda: pipeline_section(max(1, args.pipeline_reps), [int(s) for s in args.pipeline_sizes.split(",")])}
    for name in args.sections.split(","):
        res = run[name]()
        with open(os.path.join(args.out, f"{name}.json"), "w") as f:
            f.write(json.dumps(res) + "\n")
        print(json.dumps({name: res}), flush=True)


if __name__ == "__main__":
    main()
