#!/usr/bin/env python3
"""TUN frames read packed, put into slots and resolved in one launch: what the fused kernel costs beside the pair
it replaces, what the packed copy up does to the outgoing host pipeline, and what the packed read costs the
reading thread (DESIGN.md 4.5 "Outgoing frames packed on routed batches").

  device    qgcm_frames_resolve of 2^20 frames to 1 024 key slots into slots of 1536 bytes against the existing
            pair -- qgcm_gro_unpack with a table of lone buffers and the destination d_arena + 4, then
            qgcm_resolve_outgoing -- hipEvent times, warm, alternating, the median of --reps (at least 20), for
            three mixes: 1350-byte frames, lengths uniform in 36..1444, 64-byte frames; with the bytes read and
            written per second beside the rate of qgcm_stream_copy in the same run
  pipeline  qgcm_route_chain_seal_packed_host (slots in) against qgcm_route_chain_seal_frames_host in one process,
            alternating, for 65536 and 2^20 TUN packets of 1350 bytes to 1 024 peers, at stride 1536 and at stride
            9216: wall milliseconds, the median of --pipeline-reps after a warm round, the existing call's own
            spread, and the bytes that go up and come down
  tun       thread-CPU microseconds per packet inside qgcm_tun_read_packed against qgcm_tun_read_slots, bursts of
            256 datagrams of 1350 bytes through a TUN queue, alternating by burst (CPU only; needs root)

Writes one JSON file per section into --out (default profiles/frames_in) and prints them.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.send_plan_bench import PEERS, TUN_LEN, make_ctx  # noqa: E402

DGRAM = 4 + TUN_LEN + 28  # 1382


def frame_table(lens):
    """Frames back to back, each on the next 16-byte boundary -> ((n, 2) uint32, the area's size)."""
    step = (lens.astype(np.int64) + 15) & ~15
    offs = np.concatenate([[0], np.cumsum(step)[:-1]])
    return np.stack([offs, lens], axis=1).astype(np.uint32), int(offs[-1] + step[-1])


def device_section(reps):
    import torch

    from bench import GpuTelemetry, stream_copy_gbs
    from quantum_amd import route

    n, stride = 1 << 20, 1536
    ctx, addrs = make_ctx()
    rng = np.random.default_rng(0xF4A1)

    def once(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3

    def alternating(fns):
        """The median of `reps` timings of each, taken in alternating rounds after three warm ones."""
        took = {k: [] for k in fns}
        for rep in range(reps + 3):
            for k, fn in fns.items():
                us = once(fn)
                if rep >= 3:
                    took[k].append(us)
        return {k: round(statistics.median(v), 1) for k, v in took.items()}

    res = {"frames": n, "stride": stride, "max_keys": PEERS, "reps": reps}
    tel = GpuTelemetry(0)
    tel.span = "the device timings"
    tel.start()
    res["copy_achievable_gb_s"] = round(stream_copy_gbs(ctx, 1 << 30, "cuda", torch.cuda.current_stream()), 1)
    dest = torch.from_numpy(addrs[rng.integers(0, PEERS, n)].view(np.uint8).reshape(n, 4).copy()).cuda()
    whole = torch.zeros(n * stride + 16, dtype=torch.uint8, device="cuda")
    arena = whole[:n * stride]
    lens = torch.zeros(n, dtype=torch.int32, device="cuda")
    peer = torch.zeros(n, dtype=torch.int32, device="cuda")
    descs = torch.zeros(16 * n, dtype=torch.uint8, device="cuda")
    mixes = {"f1350": np.full(n, TUN_LEN, np.uint32), "f36_1444_uniform": rng.integers(36, 1445, n).astype(np.uint32),
             "f64": np.full(n, 64, np.uint32)}
    for name, h_lens in mixes.items():
        frames, size = frame_table(h_lens)
        packed = torch.randint(0, 256, (size,), dtype=torch.uint8, device="cuda")
        at = torch.from_numpy(frames[:, 0].astype(np.int64)).cuda()[:, None] + torch.arange(16, 20, device="cuda")[None, :]
        packed[at.reshape(-1)] = dest.reshape(-1)  # Packet[16:20]
        d_frames = torch.from_numpy(frames.view(np.int32).reshape(-1).copy()).cuda()
        bufs = np.stack([frames[:, 0], frames[:, 1], np.zeros(n, np.uint32), np.arange(n, dtype=np.uint32)], axis=1)
        d_bufs = torch.from_numpy(bufs.view(np.int32).reshape(-1).copy()).cuda()
        del at
        fused = lambda: route.frames_resolve(ctx, packed, size, d_frames, n, arena, stride, lens, peer, descs)
        unpack = lambda: route.gro_unpack(ctx, packed, size, d_bufs, n, n, whole[4:], stride, lens)
        resolve = lambda: route.resolve_outgoing(ctx, arena, stride, n, lens, peer, descs)

        def pair():
            unpack()
            resolve()

        us = alternating({"fused": fused, "pair": pair, "unpack": unpack, "resolve": resolve})
        fused()
        torch.cuda.synchronize()
        hits = int((peer != -1).sum())
        assert hits == n, (name, hits)
        total = int(h_lens.sum())
        # read: the frames' bytes, the table, one route entry a frame; written: the frames' bytes, own_ip, lens,
        # peer, descs
        moved = 2 * total + 8 * n + 8 * n + 4 * n + 4 * n + 4 * n + 16 * n
        res[f"{name}_frames_resolve_us"] = us["fused"]
        res[f"{name}_pair_us"] = us["pair"]
        res[f"{name}_gro_unpack_us"] = us["unpack"]
        res[f"{name}_resolve_outgoing_us"] = us["resolve"]
        res[f"{name}_pair_over_fused"] = round(us["pair"] / us["fused"], 2)
        res[f"{name}_packed_bytes"] = size
        res[f"{name}_bytes_read_plus_written"] = moved
        res[f"{name}_gb_s"] = round(moved / (us["fused"] * 1e-6) / 1e9, 1)
        res[f"{name}_share_of_copy_achievable"] = round(res[f"{name}_gb_s"] / res["copy_achievable_gb_s"], 3)
        print(json.dumps({k: v for k, v in res.items() if k.startswith(name)}), flush=True)
        del packed, d_frames, d_bufs
    tel.stop()
    res["sclk_mhz_mean"] = tel.summary().get("sclk_mhz_mean")
    ctx.close()
    return res


def pipeline_section(reps, sizes):
    from quantum_amd import batch, route

    ctx, addrs = make_ctx()
    res = {"tun_bytes": TUN_LEN, "datagram_bytes": DGRAM, "reps": reps, "cpus": len(os.sched_getaffinity(0))}
    rng = np.random.default_rng(0xF4A2)
    for n in sizes:
        dest = rng.integers(0, PEERS, n)
        pkts = rng.integers(0, 256, (4096, TUN_LEN), dtype=np.uint8)[np.arange(n) % 4096]
        pkts[:, 16:20] = addrs[dest].view(np.uint8).reshape(n, 4)
        frames, size = frame_table(np.full(n, TUN_LEN, np.uint32))
        step = size // n
        packed = np.zeros((n, step), np.uint8)
        packed[:, :TUN_LEN] = pkts
        packed = packed.reshape(-1)
        out_buf, ptrains, order = np.zeros(n * DGRAM + 16 * n, np.uint8), np.zeros((n, 4), np.uint32), np.zeros(n, np.uint32)
        for stride in (1536, 9216):
            arena = np.zeros((n, stride), np.uint8)
            arena[:, 4:4 + TUN_LEN] = pkts  # what qgcm_tun_read_slots leaves; the packed call only reads it
            peer, status = np.zeros(n, np.uint32), np.zeros(n, np.uint8)
            wall = {"slots_in": [], "frames_in": []}
            for rep in range(reps + 1):
                for which in ("slots_in", "frames_in"):
                    lens = np.full(n, TUN_LEN, np.uint32)
                    t0 = time.perf_counter()
                    if which == "slots_in":
                        dropped, pt, od, out = route.route_chain_seal_packed_host(ctx, arena.ctypes.data, stride, n, lens,
                                                                                  batch.GENERATE, route.PLUGIN_ENCRYPTION, peer,
                                                                                  status, out_buf, None, ptrains, order)
                    else:
                        dropped, pt, od, out = route.route_chain_seal_frames_host(ctx, packed, size, frames, stride, n, lens,
                                                                                  batch.GENERATE, route.PLUGIN_ENCRYPTION, peer,
                                                                                  status, out_buf, None, ptrains, order)
                    t1 = time.perf_counter()
                    t, m, used = int(out[1]), int(out[3]), int(out[2])
                    assert dropped == 0 and m == n and np.all(lens == DGRAM), (which, dropped, m)
                    if rep >= 1:  # one warm round
                        wall[which].append(t1 - t0)
            key = f"n{n}_stride{stride}"
            for which in ("slots_in", "frames_in"):
                res[f"{key}_{which}_ms"] = round(statistics.median(wall[which]) * 1e3, 2)
            res[f"{key}_slots_in_min_ms"] = round(min(wall["slots_in"]) * 1e3, 2)
            res[f"{key}_slots_in_max_ms"] = round(max(wall["slots_in"]) * 1e3, 2)
            res[f"{key}_frames_in_max_ms"] = round(max(wall["frames_in"]) * 1e3, 2)
            res[f"{key}_trains"] = t
            down = used + 16 * t + 4 * n + 9 * n
            res[f"{key}_bytes_up_slots_in"] = n * stride + 4 * n
            res[f"{key}_bytes_up_frames_in"] = size + 8 * n
            res[f"{key}_bytes_down"] = down
            res[f"{key}_byte_ratio"] = round((n * stride + 4 * n + down) / (size + 8 * n + down), 2)
            res[f"{key}_ratio_slots_in_over_frames_in"] = round(res[f"{key}_slots_in_ms"] / res[f"{key}_frames_in_ms"], 2)
            res[f"{key}_frames_in_median_below_slots_in_min"] = res[f"{key}_frames_in_ms"] < res[f"{key}_slots_in_min_ms"]
            res[f"{key}_frames_in_median_at_or_below_slots_in_max"] = res[f"{key}_frames_in_ms"] <= res[f"{key}_slots_in_max_ms"]
            print(json.dumps({k: v for k, v in res.items() if k.startswith(key)}), flush=True)
            del arena
    ctx.close()
    return res


def tun_section(total):
    from quantum_amd import _lib, common
    from tests.test_tun_batch import HOST_IP, PEER_IP

    L = _lib.lib()
    stride, batch_n, burst = common.MaxPacketLength, 512, 256
    fds, name = (C.c_int * 1)(), C.create_string_buffer(16)
    assert L.qgcm_tun_open(b"qgcmr%d", 1, fds, name, 16) == 0
    res = {"payload_bytes": TUN_LEN, "packet_bytes": TUN_LEN + 28, "burst": burst, "read_mode": os.environ.get("QGCM_TUN_URING", "")}
    try:
        assert L.qgcm_tun_up(name.value, HOST_IP.encode(), 24, 1433) == 0
        fd = fds[0]
        tx = L.qgcm_udp_socket(HOST_IP.encode(), 0, 1 << 24)
        src = np.frombuffer(os.urandom(burst * stride), dtype=np.uint8).copy()
        lens = np.full(burst, TUN_LEN, dtype=np.uint32)
        arena, rl = np.zeros(batch_n * stride, np.uint8), np.zeros(batch_n, np.uint32)
        packed, frames = np.zeros(batch_n * 1440 + 65536, np.uint8), np.zeros((batch_n, 2), np.uint32)
        while L.qgcm_tun_read_slots(fd, arena.ctypes.data, stride, batch_n, rl.ctypes.data, 20) > 0:
            pass  # link-up chatter
        reads = {"slots": lambda: L.qgcm_tun_read_slots(fd, arena.ctypes.data, stride, batch_n, rl.ctypes.data, 5),
                 "packed": lambda: L.qgcm_tun_read_packed(fd, packed.ctypes.data, packed.size, frames.ctypes.data, batch_n, 5, None)}
        got, cpu, wall, calls = {k: 0 for k in reads}, {k: 0.0 for k in reads}, {k: 0.0 for k in reads}, {k: 0 for k in reads}
        rounds = 0
        while min(got.values()) < total:
            for which, read in reads.items():
                # bursts of 256: the device's transmit queue (txqueuelen) holds 500 packets
                assert L.qgcm_udp_send_slots(tx, src.ctypes.data, stride, burst, lens.ctypes.data, PEER_IP.encode(), 9000) == burst
                seen = 0
                while seen < burst:
                    w0, c0 = time.perf_counter(), time.thread_time()
                    r = read()
                    w1, c1 = time.perf_counter(), time.thread_time()
                    if r <= 0:
                        break  # the kernel dropped the rest (queue full): count what arrived
                    seen += r
                    if rounds >= 8:  # eight warm bursts each
                        cpu[which] += c1 - c0
                        wall[which] += w1 - w0
                        calls[which] += 1
                if rounds >= 8:
                    got[which] += seen
            rounds += 1
        for which in reads:
            res[f"{which}_packets"] = got[which]
            res[f"{which}_packets_per_call"] = round(got[which] / max(1, calls[which]), 1)
            res[f"{which}_cpu_us_per_packet"] = round(cpu[which] / got[which] * 1e6, 4)
            res[f"{which}_wall_us_per_packet"] = round(wall[which] / got[which] * 1e6, 4)
        res["cpu_ratio_slots_over_packed"] = round(res["slots_cpu_us_per_packet"] / res["packed_cpu_us_per_packet"], 3)
        L.qgcm_udp_close(tx)
    finally:
        L.qgcm_tun_close(fds[0])
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--pipeline-reps", type=int, default=3)
    ap.add_argument("--pipeline-sizes", default="65536,1048576")
    ap.add_argument("--tun-packets", type=int, default=200_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames_in"))
    ap.add_argument("--sections", default="device,pipeline")
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    run = {"device": lambda: device_section(max(20, args.reps)),
           "pipeline": lambda: pipeline_section(max(1, args.pipeline_reps), [int(s) for s in args.pipeline_sizes.split(",")]),
           "tun": lambda: tun_section(args.tun_packets)}
    for name in args.sections.split(","):
        res = run[name]()
        with open(os.path.join(args.out, f"{name}.json"), "w") as f:
            f.write(json.dumps(res) + "\n")
        print(json.dumps({name: res}), flush=True)


if __name__ == "__main__":
    main()
