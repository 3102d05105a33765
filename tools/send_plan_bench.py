#!/usr/bin/env python3
"""The send plan of a routed batch: what the plan costs on the device and on the host, and what the planned
send saves on a loopback socket (DESIGN.md 4.5 "Send plan on routed batches").

  device   qgcm_send_plan of 2^20 packets, hipEvent times of one call, warm, the median of --reps (at least 20),
           for three mixes -- 1024 peers uniform with one length (1382), one peer, 1024 peers with lengths
           uniform in 64..1472 -- beside qgcm_resolve_outgoing and qgcm_seal_batch of the same batch
  host     qgcm_send_plan_cpu in ns per packet on one thread, and the wall time of qgcm_send_plan_host on its
           device path (QGCM_PLAN_DEVICE_MIN=0) and its host path (=4294967295) at n = 64 .. 2^20 by powers of
           four; "device_min" is the smallest n from which the device path stays below the host path
  send     16384 sealed 1382-byte datagrams (qgcm_route_chain_seal_host, encryption only) on loopback from one
           thread, qgcm_udp_send_slots_to against qgcm_send_plan_host + qgcm_udp_send_plan, alternating: wall
           and thread-CPU microseconds per datagram, for one peer, 16 peers round-robin and 1024 peers
           uniform; 16 receiver sockets drained by a thread (peer p sends to socket p % 16)

Writes one JSON file per section into --out (default profiles/send_plan) and prints them.
"""
from __future__ import annotations

import argparse
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

STRIDE, TUN_LEN = 1472, 1350  # the datagram is 4 + 1350 + 28 = 1382 bytes
PEERS = 1024


def make_ctx(**env):
    from quantum_amd import route
    from quantum_amd.crypto import Context

    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        ctx = Context(device=0, max_keys=PEERS)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    rng = np.random.default_rng(0x5E9D)
    ctx.set_keys(0, rng.integers(0, 256, 32 * PEERS, dtype=np.uint8).tobytes())
    addrs = np.array([10 | 99 << 8 | (j >> 8) << 16 | (j & 255) << 24 for j in range(2, 2 + PEERS)], np.uint32)
    route.routes_set(ctx, {int(a): k for k, a in enumerate(addrs)}, 10 | 99 << 8, 0xFFFF,
                     10 | 99 << 8 | 255 << 16 | 254 << 24, 10 | 99 << 8 | 1 << 24)
    return ctx, addrs


def mixes(n, rng):
    """name -> (destination peer, datagram length) per packet"""
    full = np.full(n, TUN_LEN + 32, np.uint32)
    return {"peers1024_one_length": (rng.integers(0, PEERS, n).astype(np.uint32), full),
            "one_peer": (np.zeros(n, np.uint32), full),
            "peers1024_lengths_64_1472": (rng.integers(0, PEERS, n).astype(np.uint32),
                                          rng.integers(64, 1473, n).astype(np.uint32))}


def device_section(reps):
    import torch

    from bench import GpuTelemetry
    from quantum_amd import batch, route

    n = 1 << 20
    ctx, addrs = make_ctx()
    rng = np.random.default_rng(0x91A7)
    mix = mixes(n, rng)
    dest = mix["peers1024_one_length"][0]
    arena = torch.from_numpy(rng.integers(0, 256, (4096, STRIDE), dtype=np.uint8)).cuda().repeat(n // 4096, 1).contiguous()
    arena[:, 20:24] = torch.from_numpy(addrs[dest].view(np.uint8).reshape(n, 4).copy()).cuda()
    lens = torch.full((n,), TUN_LEN, dtype=torch.int32, device="cuda")
    peer = torch.zeros(n, dtype=torch.int32, device="cuda")
    descs = torch.zeros(16 * n, dtype=torch.uint8, device="cuda")
    status = torch.zeros(n, dtype=torch.uint8, device="cuda")
    order = torch.zeros(n, dtype=torch.int32, device="cuda")
    trains = torch.zeros(4 * n, dtype=torch.int32, device="cuda")
    counts = torch.zeros(2, dtype=torch.int32, device="cuda")
    work = route.send_plan_work(n)

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

    res = {"packets": n, "max_keys": PEERS, "reps": reps, "work_bytes": int(work.numel())}
    tel = GpuTelemetry(0)
    tel.span = "the device timings"
    tel.start()
    res["resolve_outgoing_us"] = timed(lambda: route.resolve_outgoing(ctx, arena, STRIDE, n, lens, peer, descs))
    res["seal_batch_us"] = timed(lambda: batch.seal_batch(ctx, arena, descs, n, None, status=status))
    for name, (p, ln) in mix.items():
        d_peer = torch.from_numpy(p.view(np.int32).copy()).cuda()
        d_lens = torch.from_numpy(ln.view(np.int32).copy()).cuda()
        res[f"{name}_plan_us"] = timed(lambda: route.send_plan(ctx, n, d_lens, d_peer, order, trains, counts, work))
        m, t = counts.cpu().tolist()
        res[f"{name}_m"], res[f"{name}_trains"] = m, t
    tel.stop()
    res["sclk_mhz_mean"] = tel.summary().get("sclk_mhz_mean")
    ctx.close()
    return res


def host_section(reps):
    from quantum_amd import route

    rng = np.random.default_rng(0x4057)
    res = {"reps": reps, "cpus": len(os.sched_getaffinity(0)), "max_keys": PEERS}
    n = 1 << 20
    for name, (p, ln) in mixes(n, rng).items():
        ts = []
        for _ in range(7):
            t0 = time.perf_counter()
            route.send_plan_cpu(ln, p, PEERS)
            ts.append(time.perf_counter() - t0)
        res[f"cpu_{name}_ns_per_packet"] = round(statistics.median(ts) / n * 1e9, 2)
    dev_ctx, _ = make_ctx(QGCM_PLAN_DEVICE_MIN=0)
    host_ctx, _ = make_ctx(QGCM_PLAN_DEVICE_MIN=4294967295)
    sizes = [4 ** k for k in range(3, 11)]
    p_all, ln_all = mixes(n, rng)["peers1024_one_length"]
    device_min = None
    for size in sizes:
        p, ln = p_all[:size].copy(), ln_all[:size].copy()
        out = {}
        for label, c in (("device", dev_ctx), ("host", host_ctx)):
            for _ in range(3):
                route.send_plan_host(c, ln, p)
            ts = []
            for _ in range(reps if size <= 65536 else max(5, reps // 4)):
                t0 = time.perf_counter()
                route.send_plan_host(c, ln, p)
                ts.append(time.perf_counter() - t0)
            out[label] = round(statistics.median(ts) * 1e6, 1)
        res[f"host_call_n{size}_device_us"], res[f"host_call_n{size}_host_us"] = out["device"], out["host"]
        if out["device"] < out["host"]:
            device_min = size if device_min is None else device_min
        else:
            device_min = None
    res["device_min"] = device_min  # None: the device path never stays below the host path up to 2^20
    dev_ctx.close()
    host_ctx.close()
    return res


def send_section(reps):
    import ctypes as C

    from quantum_amd import _lib, batch, route

    L = _lib.lib()
    n, socks = 16384, 16
    ctx, addrs = make_ctx()
    rng = np.random.default_rng(0x5E2D)
    rx = [L.qgcm_udp_socket(b"127.0.0.1", 0, 1 << 22) for _ in range(socks)]
    tx = L.qgcm_udp_socket(b"127.0.0.1", 0, 1 << 22)
    assert tx >= 0 and all(fd >= 0 for fd in rx)
    ports = [L.qgcm_udp_port(fd) for fd in rx]
    peer_addrs = route.peer_addrs([("127.0.0.1", ports[p % socks]) for p in range(PEERS)])
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
    res = {"datagrams": n, "bytes": TUN_LEN + 32, "reps": reps, "receiver_sockets": socks, "kernel": platform.release()}
    dests = {"one_peer": np.zeros(n, np.int64), "peers16_round_robin": np.arange(n) % 16,
             "peers1024_uniform": rng.integers(0, PEERS, n)}
    size = n * STRIDE
    ptr = L.qgcm_host_alloc(size)
    assert ptr
    try:
        arena = np.frombuffer((C.c_uint8 * size).from_address(ptr), np.uint8).reshape(n, STRIDE)
        for name, dest in dests.items():
            arena[:] = rng.integers(0, 256, (n, STRIDE), dtype=np.uint8)
            arena[:, 20:24] = addrs[dest].view(np.uint8).reshape(n, 4)
            lens, peer = np.full(n, TUN_LEN, np.uint32), np.zeros(n, np.uint32)
            dropped = route.route_chain_seal_host(ctx, ptr, STRIDE, n, lens, batch.GENERATE, route.PLUGIN_ENCRYPTION, peer)
            assert dropped == 0 and np.array_equal(peer, dest.astype(np.uint32))
            t0 = time.perf_counter()
            order, trains = route.send_plan_host(ctx, lens, peer)
            res[f"{name}_plan_host_us"] = round((time.perf_counter() - t0) * 1e6, 1)
            stats = np.zeros(3, np.uint64)
            wall = {"slots_to": [], "plan": []}
            cpu = {"slots_to": [], "plan": []}
            for rep in range(reps + 2):
                for which in ("slots_to", "plan"):
                    w0, c0 = time.perf_counter(), time.thread_time()
                    if which == "plan":
                        sent = route.udp_send_plan(tx, ptr, STRIDE, n, lens, order, trains, peer_addrs, PEERS, stats)
                    else:
                        sent = route.udp_send_slots_to(tx, ptr, STRIDE, n, lens, peer, peer_addrs, PEERS)
                    w1, c1 = time.perf_counter(), time.thread_time()
                    assert sent == n, (which, sent)
                    if rep >= 2:  # two warm rounds
                        wall[which].append(w1 - w0)
                        cpu[which].append(c1 - c0)
            for which in ("slots_to", "plan"):
                res[f"{name}_{which}_wall_us_per_datagram"] = round(statistics.median(wall[which]) / n * 1e6, 4)
                res[f"{name}_{which}_cpu_us_per_datagram"] = round(statistics.median(cpu[which]) / n * 1e6, 4)
            res[f"{name}_trains"] = int(len(trains))
            res[f"{name}_stats"] = [int(v) for v in stats]
            res[f"{name}_cpu_ratio_slots_to_over_plan"] = round(
                res[f"{name}_slots_to_cpu_us_per_datagram"] / res[f"{name}_plan_cpu_us_per_datagram"], 2)
        del arena
    finally:
        stop.set()
        th.join()
        L.qgcm_host_free(ptr)
        for fd in rx + [tx]:
            L.qgcm_udp_close(fd)
        ctx.close()
    res["received_by_the_drain_thread"] = received[0]
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "send_plan"))
    ap.add_argument("--sections", default="device,host,send")
    args = ap.parse_args()
    reps = max(20, args.reps)
    os.makedirs(args.out, exist_ok=True)
    run = {"device": device_section, "host": host_section, "send": lambda r: send_section(max(10, r // 2))}
    for name in args.sections.split(","):
        res = run[name](reps)
        with open(os.path.join(args.out, f"{name}.json"), "w") as f:
            f.write(json.dumps(res) + "\n")
        print(json.dumps({name: res}), flush=True)


if __name__ == "__main__":
    main()
