#!/usr/bin/env python3
"""Delivered TCP segments coalesced for the TUN write: what the coalescing costs on the device beside the pack it
replaces, what it does to the incoming host pipeline, and what the coalesced TUN write saves the writing thread
(DESIGN.md 4.5 "Delivered TCP segments coalesced on routed batches").

  device    qgcm_deliver_coalesce against qgcm_deliver_pack on the same 2^20 slots of 1536 bytes: hipEvent times of one
            call, warm, alternating, --reps rounds (at least 20): the median with least and greatest and the mean
            clock, for 45-segment trains of 1348-byte payload, mixed flows with 10 % dropped, and lone 64-byte
            packets
  pipeline  qgcm_route_chain_open_gro_coalesced_host against qgcm_route_chain_open_gro_packed_host in one process,
            alternating, for 65536 and 2^20 sealed TCP segments in 45-segment trains: wall milliseconds, the median
            of --pipeline-reps after a warm call
  tun       thread-CPU microseconds per delivered packet inside qgcm_tun_write_gso on an offload TUN against
            qgcm_tun_write_packed on a plain one, the same delivered TCP segments -- one flow of 11 520 segments a
            batch, which the 65535-byte cut makes frames of 48 -- a local receiver draining; needs no GPU

Writes one JSON file per section into --out (default profiles/coalesce) and prints them.
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import statistics
import struct
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import coalesce_cases as K  # noqa: E402
import coalesce_model as M  # noqa: E402
from tools.send_plan_bench import make_ctx  # noqa: E402

SEGS, PAYLOAD = 45, 1348


def spread(xs):
    return {"median": round(statistics.median(xs), 1), "min": round(min(xs), 1), "max": round(max(xs), 1)}


def tile_batch(case, n, stride):
    """a batch of `n` slots from a smaller one repeated whole (trains stay trains: its length is a multiple of SEGS)"""
    arena, lens, peer, status = case
    k = len(lens)
    reps = -(-n // k)
    return (np.tile(arena.reshape(k, stride), (reps, 1))[:n].reshape(-1), np.tile(lens, reps)[:n], np.tile(peer, reps)[:n],
            np.tile(status, reps)[:n])


def device_section(reps):
    import torch

    from bench import GpuTelemetry
    from quantum_amd import route

    n, stride, base = 1 << 20, 1536, SEGS * 1024
    ctx, _ = make_ctx()
    batches = {
        "trains45_p1348": tile_batch(K.trains(base, stride, PAYLOAD, SEGS, seed=1), n, stride),
        "mixed_10pct_dropped": tile_batch(K.trains(base, stride, (1, 1400), 9, seed=2, drop=0.1), n, stride),
        "lone_64_byte": tile_batch(K.trains(base, stride, 24, 1, seed=3), n, stride),
    }
    res = {"packets": n, "stride": stride, "reps": reps}
    tel = GpuTelemetry(0)
    tel.span = "the device timings"
    tel.start()
    arena = torch.empty(n * stride, dtype=torch.uint8, device="cuda")
    out = torch.empty(n * (stride + 16), dtype=torch.uint8, device="cuda")
    frames = torch.empty(32 * n, dtype=torch.uint8, device="cuda")
    recs = torch.empty(4 * n, dtype=torch.int32, device="cuda")
    counts = torch.zeros(4, dtype=torch.int64, device="cuda")
    cwork, pwork = route.deliver_coalesce_work(n), route.deliver_pack_work(n)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3

    for name, (h_arena, h_lens, h_peer, h_status) in batches.items():
        arena.copy_(torch.from_numpy(h_arena))
        lens = torch.from_numpy(h_lens.view(np.int32)).cuda()
        peer = torch.from_numpy(h_peer.view(np.int32)).cuda()
        status = torch.from_numpy(h_status).cuda()
        calls = {"coalesce": lambda: route.deliver_coalesce(ctx, arena, stride, n, lens, peer, status, out, out.numel(), frames,
                                                            counts, cwork),
                 "pack": lambda: route.deliver_pack(ctx, arena, stride, n, lens, peer, status, out, out.numel(), recs, counts, pwork)}
        times = {"coalesce": [], "pack": []}
        for rep in range(reps + 3):  # three warm rounds
            for which in ("pack", "coalesce"):
                us = timed(calls[which])
                if rep >= 3:
                    times[which].append(us)
        calls["coalesce"]()
        torch.cuda.synchronize()
        c = counts.cpu().numpy().tolist()
        res[name] = {"coalesce_us": spread(times["coalesce"]), "pack_us": spread(times["pack"]),
                     "ratio_coalesce_over_pack": round(statistics.median(times["coalesce"]) / statistics.median(times["pack"]), 2),
                     "entries": c[0], "bytes": c[1], "coalesced_entries": c[2], "delivered": c[3]}
        print(json.dumps({name: res[name]}), flush=True)
    tel.stop()
    res["sclk_mhz_mean"] = tel.summary().get("sclk_mhz_mean")
    ctx.close()
    return res


def sealed_trains(ctx, addrs, n):
    """n sealed TCP segments of PAYLOAD bytes in SEGS-segment trains to peer 0, in slots of 1472 bytes"""
    from quantum_amd import batch, route

    stride = 1472
    f = M.fields(n)
    k = np.arange(n)
    train, at = k // SEGS, k % SEGS
    f["P"][:] = PAYLOAD
    f["seq"] = (11 + 70001 * train + at * PAYLOAD) & 0xFFFFFFFF
    f["id"] = (train * 7 + at) & 0xFFFF
    f["sport"] = 2000 + train % 30000
    f["dst"][:] = int.from_bytes(int(addrs[0]).to_bytes(4, "little"), "big")
    arena, lens = M.build(f, stride, np.random.default_rng(n))
    peer = np.zeros(n, np.uint32)
    assert route.route_chain_seal_host(ctx, arena.ctypes.data, stride, n, lens, batch.GENERATE, route.PLUGIN_ENCRYPTION, peer) == 0
    return arena.reshape(n, stride), lens


def pipeline_section(reps, sizes):
    from quantum_amd import route
    from tools.gro_recv_bench import packed_layout

    ctx, addrs = make_ctx()
    own = 10 | 99 << 8 | 1 << 24
    route.routes_set(ctx, {int(addrs[0]): 0, own: 0}, 10 | 99 << 8, 0xFFFF, 10 | 99 << 8 | 255 << 16 | 254 << 24, own)
    base = SEGS * 1456  # 65520 sealed segments, over and over
    sealed, lens = sealed_trains(ctx, addrs, base)
    dgram = int(lens[0])
    assert np.all(lens == dgram)
    res = {"datagram_bytes": dgram, "segments_per_buffer": SEGS, "reps": reps, "cpus": len(os.sched_getaffinity(0))}
    stride = 1536
    for n in sizes:
        table, packed_len, total = packed_layout([(min(SEGS, n - k), dgram, dgram) for k in range(0, n, SEGS)])
        assert total == n
        packed = np.zeros((packed_len + 15) & ~15, np.uint8)
        for off, length, _, first in table.tolist():
            idx = (first + np.arange(length // dgram)) % base
            packed[off:off + length] = sealed[idx, :dgram].reshape(-1)
        out_buf = np.zeros(n * (stride + 16), np.uint8)
        recs, frames = np.zeros((n, 4), np.uint32), np.zeros(n, route.GSO_FRAME)
        h_lens, peer, status = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint8)
        wall = {"packed": [], "coalesced": []}
        for rep in range(reps + 1):
            for which in ("packed", "coalesced"):
                t0 = time.perf_counter()
                if which == "packed":
                    dropped, got, out = route.route_chain_open_gro_packed_host(ctx, packed, packed_len, table, stride, n, h_lens,
                                                                               route.PLUGIN_ENCRYPTION, peer, status, out_buf, recs)
                else:
                    dropped, got, out = route.route_chain_open_gro_coalesced_host(ctx, packed, packed_len, table, stride, n, h_lens,
                                                                                  route.PLUGIN_ENCRYPTION, peer, status, out_buf,
                                                                                  frames)
                t1 = time.perf_counter()
                assert dropped == 0 and int(out[0]) == n, (which, dropped, out)
                if rep >= 1:
                    wall[which].append((t1 - t0) * 1e3)
                res[f"n{n}_{which}_entries"] = int(out[1])
                res[f"n{n}_{which}_bytes_down"] = int(out[2])
        for which in wall:
            res[f"n{n}_{which}_ms"] = spread(wall[which])
        res[f"n{n}_ratio_coalesced_over_packed"] = round(statistics.median(wall["coalesced"]) / statistics.median(wall["packed"]), 3)
        print(json.dumps({k: v for k, v in res.items() if k.startswith(f"n{n}_")}), flush=True)
    ctx.close()
    return res


def tcp_packet(src, dst, sport, dport, seq, ack, flags, options=b""):
    """a TCP packet without payload, checksums right: the handshake the tun section plays"""
    f = M.fields(1)
    be = lambda a: int.from_bytes(socket.inet_aton(a), "big")
    f["src"][:], f["dst"][:], f["sport"][:], f["dport"][:] = be(src), be(dst), sport, dport
    f["seq"][:], f["ack"][:], f["flags"][:], f["win"][:], f["id"][:] = seq & 0xFFFFFFFF, ack, flags, 65535, 0x4242
    f["doff"][:], f["P"][:] = 20 + len(options), 0
    arena, lens = M.build(f, 128, np.random.default_rng(0), fix=False)
    arena[44:44 + len(options)] = np.frombuffer(options, np.uint8)
    M.fix_checksums(arena, 128, 0, lens)
    return arena[4:4 + int(lens[0])].tobytes()


def tun_section(reps):
    import ctypes as C

    from quantum_amd import _lib, route

    L = _lib.lib()
    host, peer_ip = "10.213.12.1", "10.213.12.2"
    n, stride = 256 * SEGS, 1536  # one flow: as many segments as 256 trains hold
    res = {"packets": n, "flows": 1, "payload": PAYLOAD, "reps": reps, "machine": "the build machine (no GPU)"}

    def be(ip):
        return int.from_bytes(socket.inet_aton(ip), "big")

    def measure(offload):
        if offload:
            rc, fds, name = route.tun_open_offload(b"qgcmb%d", 1, _lib.TUN_TSO4)
        else:
            fds, namebuf = (C.c_int * 1)(), C.create_string_buffer(16)
            rc = L.qgcm_tun_open(b"qgcmb%d", 1, fds, namebuf, 16)
            name = namebuf.value
        if rc < 0:
            return None, f"TUN device refused (errno {-rc})"
        fd = fds[0]
        srv = socket.socket(socket.AF_INET, socket.SOCK_STREAM)
        try:
            if L.qgcm_tun_up(name, host.encode(), 24, 1433) < 0:
                return None, "TUN link set-up refused"
            srv.setsockopt(socket.SOL_SOCKET, socket.SO_REUSEADDR, 1)
            srv.setsockopt(socket.SOL_SOCKET, socket.SO_RCVBUF, 1 << 24)
            srv.bind((host, 0))
            srv.listen(1)
            srv.settimeout(5)
            port, sport, isn = srv.getsockname()[1], 40321, 0x9000
            lead = 10 if offload else 0

            def raw_write(pkt):
                return os.write(fd, bytes(lead) + pkt)

            def raw_read():
                return os.read(fd, 70000)[lead:]

            raw_write(tcp_packet(peer_ip, host, sport, port, isn, 0, 0x02, struct.pack("!BBHBBB", 2, 4, 1393, 3, 3, 9) + b"\x01"))
            their = None
            for _ in range(50):
                p = raw_read()
                if len(p) >= 40 and p[9] == 6 and p[33] == 0x12:
                    their = struct.unpack("!I", p[24:28])[0]
                    break
            if their is None:
                return None, "no SYN-ACK"
            ack = (their + 1) & 0xFFFFFFFF
            raw_write(tcp_packet(peer_ip, host, sport, port, isn + 1, ack, 0x10))
            conn, _ = srv.accept()
            got = [0]

            def drain():
                while True:
                    try:
                        b = conn.recv(1 << 20)
                    except OSError:
                        return
                    if not b:
                        return
                    got[0] += len(b)

            threading.Thread(target=drain, daemon=True).start()

            def reader():  # the ACKs the stack sends back must leave the queue
                while True:
                    try:
                        os.read(fd, 70000)
                    except OSError:
                        return

            threading.Thread(target=reader, daemon=True).start()
            cpu, seq = [], isn + 1
            for rep in range(reps + 1):
                f = M.fields(n)
                M.run(f, 0, n, PAYLOAD, seq0=seq, id0=rep * n)
                f["src"][:], f["dst"][:], f["sport"][:], f["dport"][:], f["ack"][:], f["win"][:] = be(peer_ip), be(host), sport, port, ack, 65535
                arena, lens = M.build(f, stride, np.random.default_rng(rep))
                zeros = np.zeros(n, np.uint32)
                if offload:
                    packed = np.zeros(n * (stride + 16), np.uint8)
                    frames, counts = route.deliver_coalesce_cpu(arena, stride, n, lens, zeros, None, packed)
                    assert int(counts[2]) == len(frames)  # one flow: the cut makes frames of (65535 - 40) / 1348 = 48
                    res["segments_per_entry_max"] = int(frames["count"].max())
                    out = np.zeros(3, np.uint64)
                    c0 = time.thread_time()
                    wrote = route.tun_write_gso(fd, packed, int(counts[1]), frames, out)
                    c1 = time.thread_time()
                    assert wrote == len(frames) and int(out[1]) == n, (wrote, out)
                    res["entries_that_fell_back"] = res.get("entries_that_fell_back", 0) + int(out[2])
                    res["entries_per_batch"] = len(frames)
                else:
                    packed = np.zeros(n * stride, np.uint8)
                    recs, total = route.deliver_pack_cpu(arena, stride, n, lens, zeros, None, packed)
                    c0 = time.thread_time()
                    wrote = route.tun_write_packed(fd, packed, total, recs)
                    c1 = time.thread_time()
                    assert wrote == n
                seq = (seq + n * PAYLOAD) & 0xFFFFFFFF
                if rep >= 1:
                    cpu.append((c1 - c0) / n * 1e6)
                deadline = time.time() + 5
                while got[0] < (rep + 1) * n * PAYLOAD and time.time() < deadline:
                    time.sleep(0.002)
            raw_write(tcp_packet(peer_ip, host, sport, port, seq, ack, 0x14))
            conn.close()
            return {"cpu_us_per_delivered_packet": round(statistics.median(cpu), 4), "min": round(min(cpu), 4), "max": round(max(cpu), 4),
                    "bytes_received_of_sent": [got[0], (reps + 1) * n * PAYLOAD]}, None
        finally:
            srv.close()
            L.qgcm_tun_close(fd)

    for key, offload in (("write_packed_plain_tun", False), ("write_gso_offload_tun", True)):
        got, why = measure(offload)
        if got is None:
            return {"measured": False, "why": why}
        res[key] = got
    res["measured"] = True
    res["ratio_packed_over_gso"] = round(res["write_packed_plain_tun"]["cpu_us_per_delivered_packet"] /
                                         res["write_gso_offload_tun"]["cpu_us_per_delivered_packet"], 2)
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--pipeline-reps", type=int, default=3)
    ap.add_argument("--pipeline-sizes", default="65536,1048576")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coalesce"))
    ap.add_argument("--sections", default="device,pipeline,tun")
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    run = {"device": lambda: device_section(max(20, args.reps)),
           "pipeline": lambda: pipeline_section(max(1, args.pipeline_reps), [int(s) for s in args.pipeline_sizes.split(",")]),
           "tun": lambda: tun_section(5)}
    for name in args.sections.split(","):
        res = run[name]()
        with open(os.path.join(args.out, f"{name}.json"), "w") as f:
            f.write(json.dumps(res) + "\n")
        print(json.dumps({name: res}), flush=True)


if __name__ == "__main__":
    main()
