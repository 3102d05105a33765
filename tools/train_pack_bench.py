#!/usr/bin/env python3
"""The trains of a planned batch packed on the GPU: what the pack costs on the device, what it does to the outgoing
host pipeline, and what one iovec a train saves the sending thread (DESIGN.md 4.5 "Planned trains packed on
routed batches").

  device    qgcm_train_pack of 2^20 datagrams of 1 024 key slots in slots of 1536 bytes, hipEvent times of one call
            (its four kernels), warm, the median of --reps (at least 20), for three plans -- 1382-byte datagrams in
            full trains, lengths uniform in 64..1472 (mostly trains of one), 64-byte datagrams -- with the bytes
            read and written per second beside the rate of qgcm_stream_copy in the same run, and qgcm_deliver_pack
            (1354-byte packets), qgcm_send_plan and the seal of the same batch beside them
  pipeline  qgcm_route_chain_seal_host + qgcm_send_plan_host against qgcm_route_chain_seal_packed_host in one
            process, alternating, for 65536 and 2^20 TUN packets of 1350 bytes to 1 024 peers, at stride 1536 and
            at stride 9216: wall milliseconds, the median of --pipeline-reps after a warm round, the existing
            pair's own spread, and the bytes that come down
  sender    thread-CPU microseconds per datagram of qgcm_udp_send_packed against qgcm_udp_send_plan for the three
            mixes of tools/send_plan_bench.py (16 384 x 1382 B on loopback, where the receive side stays per
            datagram)

Writes one JSON file per section into --out (default profiles/train_pack) and prints them.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import platform
import statistics
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.send_plan_bench import PEERS, TUN_LEN, make_ctx  # noqa: E402

DGRAM = 4 + TUN_LEN + 28  # 1382


def device_section(reps):
    import torch

    from bench import GpuTelemetry, stream_copy_gbs
    from quantum_amd import batch, route

    n, stride = 1 << 20, 1536
    ctx, addrs = make_ctx()
    rng = np.random.default_rng(0x7A41)

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

    res = {"datagrams": n, "stride": stride, "max_keys": PEERS, "reps": reps}
    tel = GpuTelemetry(0)
    tel.span = "the device timings"
    tel.start()
    res["copy_achievable_gb_s"] = round(stream_copy_gbs(ctx, 1 << 30, "cuda", torch.cuda.current_stream()), 1)
    dest = rng.integers(0, PEERS, n).astype(np.uint32)
    arena = torch.from_numpy(rng.integers(0, 256, (4096, stride), dtype=np.uint8)).cuda().repeat(n // 4096, 1).contiguous()
    arena[:, 20:24] = torch.from_numpy(addrs[dest].view(np.uint8).reshape(n, 4).copy()).cuda()
    lens = torch.full((n,), TUN_LEN, dtype=torch.int32, device="cuda")
    peer = torch.zeros(n, dtype=torch.int32, device="cuda")
    descs = torch.zeros(16 * n, dtype=torch.uint8, device="cuda")
    status = torch.ones(n, dtype=torch.uint8, device="cuda")
    res["resolve_outgoing_us"] = timed(lambda: route.resolve_outgoing(ctx, arena, stride, n, lens, peer, descs))
    res["seal_batch_us"] = timed(lambda: batch.seal_batch(ctx, arena, descs, n, None, status=status))
    del descs
    out = torch.zeros(n * stride, dtype=torch.uint8, device="cuda")
    table = torch.zeros(4 * n, dtype=torch.int32, device="cuda")
    counts64 = torch.zeros(2, dtype=torch.int64, device="cuda")
    # the aligned pack of the same slots, for the yardstick: 1354-byte packets, all delivered
    lens.fill_(1354)
    status.fill_(1)
    pwork = route.deliver_pack_work(n)
    res["deliver_pack_l1354_us"] = timed(lambda: route.deliver_pack(ctx, arena, stride, n, lens, peer, status, out, n * stride,
                                                                    table, counts64, pwork))
    moved = 2 * int(counts64.cpu()[1]) + n * (2 * 5 + 4) + 2 * 16 * n
    res["deliver_pack_l1354_gb_s"] = round(moved / (res["deliver_pack_l1354_us"] * 1e-6) / 1e9, 1)
    order = torch.zeros(n, dtype=torch.int32, device="cuda")
    trains = torch.zeros(4 * n, dtype=torch.int32, device="cuda")
    counts = torch.zeros(2, dtype=torch.int32, device="cuda")
    work, twork = route.send_plan_work(n), route.train_pack_work(n)
    inputs = {"d1382_full_trains": np.full(n, DGRAM, np.uint32),
              "d64_1472_uniform": rng.integers(64, 1473, n).astype(np.uint32),
              "d64": np.full(n, 64, np.uint32)}
    d_peer = torch.from_numpy(dest.view(np.int32).copy()).cuda()
    for name, h_lens in inputs.items():
        lens.copy_(torch.from_numpy(h_lens.view(np.int32)))
        res[f"{name}_plan_us"] = timed(lambda: route.send_plan(ctx, n, lens, d_peer, order, trains, counts, work))
        us = timed(lambda: route.train_pack(ctx, arena, stride, n, order, trains, counts, out, n * stride, table, counts64,
                                            twork))
        m, t = counts.cpu().tolist()
        t2, total = (int(v) for v in counts64.cpu().numpy())
        assert m == n and t2 == t and total >= int(h_lens.sum())
        # read: the datagrams' bytes, order once, the plan's table by the two scan passes and (about twice a
        # datagram group) by the search, the packed table by the copy; written: the packed bytes and the table
        moved = int(h_lens.sum()) + total + 4 * m + 16 * t * 2 + 2 * 16 * m + 16 * m + 16 * t
        res[f"{name}_pack_us"] = us
        res[f"{name}_trains"] = t
        res[f"{name}_packed_bytes"] = total
        res[f"{name}_bytes_read_plus_written"] = moved
        res[f"{name}_gb_s"] = round(moved / (us * 1e-6) / 1e9, 1)
        res[f"{name}_share_of_copy_achievable"] = round(res[f"{name}_gb_s"] / res["copy_achievable_gb_s"], 3)
    res["d1382_pack_us_over_deliver_pack_l1354_us"] = round(res["d1382_full_trains_pack_us"] / res["deliver_pack_l1354_us"], 2)
    tel.stop()
    res["sclk_mhz_mean"] = tel.summary().get("sclk_mhz_mean")
    ctx.close()
    return res


def pipeline_section(reps, sizes):
    from quantum_amd import batch, route

    ctx, addrs = make_ctx()
    res = {"tun_bytes": TUN_LEN, "datagram_bytes": DGRAM, "reps": reps, "cpus": len(os.sched_getaffinity(0))}
    rng = np.random.default_rng(0x7A42)
    for n in sizes:
        dest = rng.integers(0, PEERS, n)
        head = rng.integers(0, 256, (4096, DGRAM + 2), dtype=np.uint8)[np.arange(n) % 4096]
        head[:, 20:24] = addrs[dest].view(np.uint8).reshape(n, 4)
        out_buf, ptrains, order = np.zeros(n * DGRAM + 16 * n, np.uint8), np.zeros((n, 4), np.uint32), np.zeros(n, np.uint32)
        for stride in (1536, 9216):
            arena = np.zeros((n, stride), np.uint8)
            peer, status = np.zeros(n, np.uint32), np.zeros(n, np.uint8)
            wall = {"slots_out": [], "packed_out": []}
            for rep in range(reps + 1):
                for which in ("slots_out", "packed_out"):
                    arena[:, :DGRAM + 2] = head  # the existing call seals in place: the TUN packets again
                    lens = np.full(n, TUN_LEN, np.uint32)
                    t0 = time.perf_counter()
                    if which == "slots_out":
                        dropped = route.route_chain_seal_host(ctx, arena.ctypes.data, stride, n, lens, batch.GENERATE,
                                                              route.PLUGIN_ENCRYPTION, peer, status)
                        got_order, got_trains = route.send_plan_host(ctx, lens, peer)
                        t, m = len(got_trains), len(got_order)
                    else:
                        dropped, pt, od, out = route.route_chain_seal_packed_host(ctx, arena.ctypes.data, stride, n, lens,
                                                                                  batch.GENERATE, route.PLUGIN_ENCRYPTION, peer,
                                                                                  status, out_buf, None, ptrains, order)
                        t, m, used = int(out[1]), int(out[3]), int(out[2])
                    t1 = time.perf_counter()
                    assert dropped == 0 and m == n and np.all(lens == DGRAM), (which, dropped, m)
                    if rep >= 1:  # one warm round
                        wall[which].append(t1 - t0)
            key = f"n{n}_stride{stride}"
            for which in ("slots_out", "packed_out"):
                res[f"{key}_{which}_ms"] = round(statistics.median(wall[which]) * 1e3, 2)
            res[f"{key}_slots_out_min_ms"] = round(min(wall["slots_out"]) * 1e3, 2)
            res[f"{key}_slots_out_max_ms"] = round(max(wall["slots_out"]) * 1e3, 2)
            res[f"{key}_packed_out_max_ms"] = round(max(wall["packed_out"]) * 1e3, 2)
            res[f"{key}_trains"] = t
            res[f"{key}_bytes_down_slots_out"] = n * stride + 9 * n + 4 * n + 16 * t
            res[f"{key}_bytes_down_packed_out"] = used + 16 * t + 4 * n + 9 * n
            res[f"{key}_ratio_slots_out_over_packed_out"] = round(res[f"{key}_slots_out_ms"] / res[f"{key}_packed_out_ms"], 2)
            print(json.dumps({k: v for k, v in res.items() if k.startswith(key)}), flush=True)
            del arena
    ctx.close()
    return res


def sender_section(reps):
    from quantum_amd import _lib, batch, route
    from tools.send_plan_bench import STRIDE

    L = _lib.lib()
    n, socks = 16384, 16
    ctx, addrs = make_ctx()
    rng = np.random.default_rng(0x7A43)
    rx = [L.qgcm_udp_socket(b"127.0.0.1", 0, 1 << 22) for _ in range(socks)]
    tx = L.qgcm_udp_socket(b"127.0.0.1", 0, 1 << 22)
    assert tx >= 0 and all(fd >= 0 for fd in rx)
    peer_addrs = route.peer_addrs([("127.0.0.1", L.qgcm_udp_port(rx[p % socks])) for p in range(PEERS)])
    stop, received = threading.Event(), [0]

    def drain():
        buf, ln = np.zeros((1024, STRIDE), np.uint8), np.zeros(1024, np.uint32)
        while not stop.is_set():
            for fd in rx:
                r = L.qgcm_udp_recv_slots(fd, buf.ctypes.data, STRIDE, 1024, ln.ctypes.data, 0)
                if r > 0:
                    received[0] += r

    th = threading.Thread(target=drain, daemon=True)
    th.start()
    res = {"datagrams": n, "bytes": DGRAM, "reps": reps, "receiver_sockets": socks, "kernel": platform.release()}
    dests = {"one_peer": np.zeros(n, np.int64), "peers16_round_robin": np.arange(n) % 16,
             "peers1024_uniform": rng.integers(0, PEERS, n)}
    try:
        for name, dest in dests.items():
            tun = rng.integers(0, 256, (n, STRIDE), dtype=np.uint8)
            tun[:, 20:24] = addrs[dest].view(np.uint8).reshape(n, 4)
            arena, lens, peer = tun.copy(), np.full(n, TUN_LEN, np.uint32), np.zeros(n, np.uint32)
            assert route.route_chain_seal_host(ctx, arena.ctypes.data, STRIDE, n, lens, batch.GENERATE, route.PLUGIN_ENCRYPTION, peer) == 0
            order, trains = route.send_plan_host(ctx, lens, peer)
            out_buf, lens2, peer2 = np.zeros(n * STRIDE, np.uint8), np.full(n, TUN_LEN, np.uint32), np.zeros(n, np.uint32)
            rc, ptrains, _, out = route.route_chain_seal_packed_host(ctx, tun.ctypes.data, STRIDE, n, lens2, batch.GENERATE,
                                                                     route.PLUGIN_ENCRYPTION, peer2, None, out_buf)
            assert rc == 0 and len(ptrains) == len(trains) and int(out[3]) == n
            ptrains, used = np.ascontiguousarray(ptrains), int(out[2])
            stats = np.zeros(3, np.uint64)
            cpu, wall = {"plan": [], "packed": []}, {"plan": [], "packed": []}
            for rep in range(reps + 2):
                for which in ("plan", "packed"):
                    w0, c0 = time.perf_counter(), time.thread_time()
                    if which == "plan":
                        sent = route.udp_send_plan(tx, arena.ctypes.data, STRIDE, n, lens, order, trains, peer_addrs, PEERS, stats)
                    else:
                        sent = route.udp_send_packed(tx, out_buf, used, ptrains, peer_addrs, PEERS, stats)
                    w1, c1 = time.perf_counter(), time.thread_time()
                    assert sent == n, (which, sent)
                    if rep >= 2:  # two warm rounds
                        wall[which].append(w1 - w0)
                        cpu[which].append(c1 - c0)
            for which in ("plan", "packed"):
                res[f"{name}_{which}_wall_us_per_datagram"] = round(statistics.median(wall[which]) / n * 1e6, 4)
                res[f"{name}_{which}_cpu_us_per_datagram"] = round(statistics.median(cpu[which]) / n * 1e6, 4)
            res[f"{name}_trains"] = int(len(trains))
            res[f"{name}_stats"] = [int(v) for v in stats]
            res[f"{name}_cpu_ratio_plan_over_packed"] = round(
                res[f"{name}_plan_cpu_us_per_datagram"] / res[f"{name}_packed_cpu_us_per_datagram"], 2)
    finally:
        stop.set()
        th.join()
        for fd in rx + [tx]:
            L.qgcm_udp_close(fd)
        ctx.close()
    res["received_by_the_drain_thread"] = received[0]
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--pipeline-reps", type=int, default=3)
    ap.add_argument("--pipeline-sizes", default="65536,1048576")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_pack"))
    ap.add_argument("--sections", default="device,pipeline,sender")
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    run = {"device": lambda: device_section(max(20, args.reps)),
           "pipeline": lambda: pipeline_section(max(1, args.pipeline_reps), [int(s) for s in args.pipeline_sizes.split(",")]),
           "sender": lambda: sender_section(max(5, args.reps // 2))}
    for name in args.sections.split(","):
        res = run[name]()
        with open(os.path.join(args.out, f"{name}.json"), "w") as f:
            f.write(json.dumps(res) + "\n")
        print(json.dumps({name: res}), flush=True)


if __name__ == "__main__":
    main()
