#!/usr/bin/env python3
"""TUN super-frames cut into slots on the GPU: what the fused launch costs beside the parent's launch on packets
that are already segmented, what the super-frame read costs the reading thread beside the packed read, and what
the pipeline costs beside the packed-frames one (DESIGN.md 4.5 "TUN super-frames segmented on routed batches").
No ratio here is a gate: nothing existing switches to the new path.

  device    qgcm_gso_resolve of 2^20 slots into slots of 1536 bytes against qgcm_frames_resolve given the same
            packets already segmented (what the parent runs after the kernel's own software segmentation) --
            hipEvent times, warm, alternating, the median, least and greatest of --reps (at least 20) -- for three
            tables: 45-segment TCP frames of gso_size 1348, mixed frames (TCP and UDP of 1..45 segments of 536, 1348
            or 1448 bytes, CSUM and PLAIN singles), lone 64-byte PLAIN entries; the outputs of the two compared
  tun       thread-CPU microseconds per delivered packet inside qgcm_tun_read_gso on an offload TUN against
            qgcm_tun_read_packed on a plain TUN, under the same local TCP sender (a socket whose peer is this
            process: it answers the SYN and acknowledges what it reads, by packets written to the TUN) (CPU only;
            needs root)
  pipeline  qgcm_route_chain_seal_gso_host against qgcm_route_chain_seal_frames_host on the same packets already
            segmented, in one process, alternating, at 65536 and 2^20 packets of 1388 bytes: wall milliseconds,
            median, least and greatest of --pipeline-reps after a warm round, and the bytes that go up

Writes one JSON file per section into --out (default profiles/tun_gso) and prints them.
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

import gso_model as M  # noqa: E402

STRIDE = 1536


def spread(v):
    return {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}


def tables(n, addrs, which, seed):
    """(packed, packed_len, frames) naming exactly n slots: a pool of 64 frames to distinct peers, repeated."""
    rng = np.random.default_rng(seed)
    pool = []
    for j in range(64):
        dst = int(addrs[rng.integers(0, len(addrs))])
        if which == "tcp45":
            pool.append(M.tcp_frame(rng, 45 * 1348, 1348, dst, ident=int(rng.integers(0, 65536))))
        elif which == "plain64":
            pool.append(M.plain_packet(rng, 64, dst))
        else:
            pick, gso, count = j % 8, (536, 1348, 1448)[j % 3], int(rng.integers(1, 46))
            if pick < 5:
                pool.append(M.tcp_frame(rng, count * gso - int(rng.integers(0, gso)), gso, dst, tcp_hl=(20, 32)[j % 2]))
            elif pick == 5:
                pool.append(M.udp_frame(rng, count * gso - int(rng.integers(0, gso)), min(gso, 1472), dst))
            elif pick == 6:
                pool.append(M.csum_packet(rng, int(rng.integers(1, 1400)), dst, j % 16 == 6))
            else:
                pool.append(M.plain_packet(rng, int(rng.integers(20, 1400)), dst))
    step = max((len(b) + 10 + 15) & ~15 for b, _ in pool)
    blob = np.zeros((64, step), np.uint8)
    one = np.zeros(64, M.FRAME)
    for j, (b, f) in enumerate(pool):
        blob[j, 16:16 + len(b)] = b
        one[j] = M.entry(off=j * step + 16, len=len(b), first=0, **f)
    per = int(one["count"].sum())
    rounds = -(-n // per)
    frames = np.tile(one, rounds)
    frames["off"] = (frames["off"].astype(np.int64) + np.repeat(np.arange(rounds, dtype=np.int64) * 64 * step, 64)).astype(np.uint32)
    first = np.concatenate([[0], np.cumsum(frames["count"].astype(np.int64))[:-1]])
    keep = int(np.searchsorted(first + frames["count"], n, side="right"))
    frames, first = frames[:keep].copy(), first[:keep]
    frames["first"] = first
    have = int(frames["count"].sum())
    packed = np.tile(blob.reshape(-1), -(-(keep) // 64))[:(-(-keep // 64)) * 64 * step]
    if have < n:  # lone PLAIN entries of length 0 make up the count
        pad = np.zeros(n - have, M.FRAME)
        pad["count"], pad["first"] = 1, np.arange(have, n)
        frames = np.concatenate([frames, pad])
    assert (int(frames["off"].max()) if len(frames) else 0) < (1 << 32)
    return packed, packed.size, frames


def device_section(reps):
    import torch

    from bench import GpuTelemetry
    from quantum_amd import route
    from tools.send_plan_bench import make_ctx

    n = 1 << 20
    ctx, addrs = make_ctx()

    def once(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3

    res = {"slots": n, "stride": STRIDE, "reps": reps}
    tel = GpuTelemetry(0)
    tel.span = "the device timings"
    tel.start()
    whole = torch.zeros(n * STRIDE, dtype=torch.uint8, device="cuda")
    ref = torch.zeros(n * STRIDE, dtype=torch.uint8, device="cuda")
    outs = [[torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda"),
             torch.zeros(16 * n, dtype=torch.uint8, device="cuda")] for _ in range(2)]
    for which in ("tcp45", "mixed", "plain64"):
        packed, packed_len, frames = tables(n, addrs, which, 0x650 + len(which))
        d_packed = torch.from_numpy(packed).cuda()
        d_frames = torch.from_numpy(frames.view(np.uint8).reshape(-1).copy()).cuda()
        gso = lambda: route.gso_resolve(ctx, d_packed, packed_len, d_frames, len(frames), n, whole, STRIDE, *outs[0])
        gso()
        torch.cuda.synchronize()
        # the same packets already segmented, each on a 16-byte boundary at a uniform step: the parent's input (the
        # kernel reads only the pieces that hold a frame's bytes, so the step is not part of what it moves)
        lens = outs[0][0].cpu().numpy().view(np.uint32).astype(np.int64)
        assert lens.max() <= STRIDE - 32
        step = (int(lens.max()) + 15) & ~15
        size = n * step
        seg = whole.view(n, STRIDE)[:, 4:4 + step].contiguous().view(-1)
        offs = np.arange(n, dtype=np.int64) * step
        table = torch.from_numpy(np.stack([offs, lens], axis=1).astype(np.uint32).view(np.int32).reshape(-1).copy()).cuda()
        parent = lambda: route.frames_resolve(ctx, seg, size, table, n, ref, STRIDE, *outs[1])
        parent()
        torch.cuda.synchronize()
        same = all(torch.equal(a, b) for a, b in zip(outs[0], outs[1]))
        m = whole.view(n, STRIDE)
        r = ref.view(n, STRIDE)
        keep = torch.arange(STRIDE, device="cuda")[None, :] < (4 + torch.from_numpy(lens).cuda())[:, None]
        same = same and bool(((m == r) | ~keep).all())
        del keep
        took = {"gso": [], "parent": []}
        for rep in range(reps + 3):
            for k, fn in (("gso", gso), ("parent", parent)):
                us = once(fn)
                if rep >= 3:
                    took[k].append(us)
        res[which] = {"entries": len(frames), "packed_bytes": packed_len, "segmented_bytes": int(lens.sum()), "outputs_equal": same,
                      "gso_resolve_us": spread(took["gso"]), "frames_resolve_us": spread(took["parent"]),
                      "gso_over_parent": round(statistics.median(took["gso"]) / statistics.median(took["parent"]), 3)}
        print(json.dumps({which: res[which]}), flush=True)
        del d_packed, d_frames, seg, table
    tel.stop()
    res["sclk_mhz_mean"] = tel.summary().get("sclk_mhz_mean")
    ctx.close()
    return res


def pipeline_section(reps, sizes):
    from quantum_amd import batch, route
    from tools.send_plan_bench import make_ctx

    ctx, addrs = make_ctx()
    res = {"stride": STRIDE, "reps": reps, "cpus": len(os.sched_getaffinity(0))}
    for n in sizes:
        packed, packed_len, frames = tables(n, addrs, "tcp45", 0x651)
        frames = frames[frames["len"] > 0].copy()  # whole frames only: the size rounded down to a multiple of 45
        n = int(frames["count"].sum())
        arena, lens = np.zeros(n * STRIDE, np.uint8), np.zeros(n, np.uint32)
        route.gso_unpack_cpu(packed, packed_len, frames, n, arena, STRIDE, lens)
        step = (int(lens.max()) + 15) & ~15  # every packet on a 16-byte boundary, at a uniform step
        size = n * step
        seg = np.ascontiguousarray(arena.reshape(n, STRIDE)[:, 4:4 + step]).reshape(-1)
        offs = np.arange(n, dtype=np.int64) * step
        del arena
        table = np.stack([offs, lens], axis=1).astype(np.uint32)
        out_buf, ptrains, order = np.zeros(n * 1456, np.uint8), np.zeros((n, 4), np.uint32), np.zeros(n, np.uint32)
        peer, status, out_lens = np.zeros(n, np.uint32), np.zeros(n, np.uint8), np.zeros(n, np.uint32)
        wall = {"gso": [], "frames": []}
        for rep in range(reps + 1):
            for which in ("frames", "gso"):
                t0 = time.perf_counter()
                if which == "gso":
                    rc, pt, od, out = route.route_chain_seal_gso_host(ctx, packed, packed_len, frames, STRIDE, n, out_lens,
                                                                      batch.GENERATE, route.PLUGIN_ENCRYPTION, peer, status, out_buf,
                                                                      None, ptrains, order)
                else:
                    rc, pt, od, out = route.route_chain_seal_frames_host(ctx, seg, size, table, STRIDE, n, out_lens, batch.GENERATE,
                                                                         route.PLUGIN_ENCRYPTION, peer, status, out_buf, None, ptrains,
                                                                         order)
                t1 = time.perf_counter()
                assert rc == 0 and int(out[3]) == n, (which, rc, out.tolist())
                if rep >= 1:
                    wall[which].append((t1 - t0) * 1e3)
        res[f"n{n}"] = {"entries": len(frames), "bytes_up_gso": packed_len + 32 * len(frames), "bytes_up_frames": int(lens.sum()) + 8 * n,
                        "gso_ms": spread(wall["gso"]), "frames_ms": spread(wall["frames"]),
                        "gso_over_frames": round(statistics.median(wall["gso"]) / statistics.median(wall["frames"]), 3)}
        print(json.dumps({f"n{n}": res[f"n{n}"]}), flush=True)
    ctx.close()
    return res


def tcp_reply(src, dst, sport, dport, seq, ack, flags, options=b""):
    hl = 20 + len(options)
    t = bytearray(struct.pack("!HHIIBBHHH", sport, dport, seq, ack, (hl // 4) << 4, flags, 65535, 0, 0) + options)
    ip = bytearray(struct.pack("!BBHHHBBH4s4s", 0x45, 0, 20 + hl, 0, 0x4000, 64, 6, 0, socket.inet_aton(src), socket.inet_aton(dst)))
    ip[10:12] = M.rfc1071(bytes(ip)).to_bytes(2, "big")
    t[16:18] = M.rfc1071(bytes(ip[12:20]) + bytes([0, 6]) + hl.to_bytes(2, "big") + bytes(t)).to_bytes(2, "big")
    return bytes(ip) + bytes(t)


def tun_section(total_bytes):
    from quantum_amd import _lib, route

    L = _lib.lib()
    res = {"sent_bytes": total_bytes, "mtu": 1433}
    for which, host, peer_ip in (("packed", "10.213.11.1", "10.213.11.2"), ("gso", "10.213.12.1", "10.213.12.2")):
        if which == "gso":
            rc, fds, name = route.tun_open_offload(b"qgcmb%d", 1, _lib.TUN_TSO4)
            assert rc == 0, rc
        else:
            import ctypes as C

            cf, nm = (C.c_int * 1)(), C.create_string_buffer(16)
            assert L.qgcm_tun_open(b"qgcmb%d", 1, cf, nm, 16) == 0
            fds, name = [cf[0]], nm.value
        fd = fds[0]
        try:
            assert L.qgcm_tun_up(name, host.encode(), 24, 1433) == 0
            vnet = bytes(10) if which == "gso" else b""
            packed = np.zeros(1 << 22, np.uint8)
            gframes, pframes = np.zeros(64, M.FRAME), np.zeros((4096, 2), np.uint32)
            out = np.zeros(3, np.uint64)
            client = socket.socket(socket.AF_INET, socket.SOCK_STREAM)
            client.bind((host, 0))
            sender = threading.Thread(target=lambda: (client.connect((peer_ip, 9500)), client.sendall(bytes(total_bytes))), daemon=True)
            sender.start()
            cpu = wall = 0.0
            calls = packets = 0
            state = {"isn": None, "sport": 0, "next": 0, "got": 0}
            idle = 0
            while state["got"] < total_bytes and idle < 200:
                w0, c0 = time.perf_counter(), time.thread_time()
                if which == "gso":
                    n = route.tun_read_gso(fd, packed, gframes, 8192, 10, out)
                    spans = [(int(f["off"]), int(f["len"]), int(f["count"])) for f in gframes[:int(out[0])]] if n > 0 else []
                else:
                    n = route.tun_read_packed(fd, packed, pframes, 4096, 10, out)
                    spans = [(int(o), int(l), 1) for o, l in pframes[:max(n, 0)]]
                w1, c1 = time.perf_counter(), time.thread_time()
                assert n >= 0
                idle = idle + 1 if n == 0 else 0
                data_packets = 0
                for off, length, count in spans:
                    p = packed[off:off + min(length, 80)].tobytes()
                    if length < 40 or p[0] >> 4 != 4 or p[9] != 6:
                        continue
                    sport, seq, flags = struct.unpack("!H", p[20:22])[0], struct.unpack("!I", p[24:28])[0], p[33]
                    if flags & 0x02:
                        state.update(isn=seq, sport=sport, next=(seq + 1) & 0xFFFFFFFF)
                        os.write(fd, vnet + tcp_reply(peer_ip, host, 9500, sport, 0x1000, state["next"], 0x12,
                                                      struct.pack("!BBH", 2, 4, 1393)))
                        continue
                    body = length - 20 - 4 * (p[32] >> 4)
                    if body > 0 and seq == state["next"]:
                        state["next"] = (seq + body) & 0xFFFFFFFF
                        state["got"] += body
                        data_packets += count
                if data_packets:
                    os.write(fd, vnet + tcp_reply(peer_ip, host, 9500, state["sport"], 0x1001, state["next"], 0x10))
                    cpu += c1 - c0
                    wall += w1 - w0
                    calls += 1
                    packets += data_packets
            client.close()
            res[which] = {"received_bytes": state["got"], "packets": packets, "read_calls": calls,
                          "packets_per_call": round(packets / max(1, calls), 1),
                          "cpu_us_per_packet": round(cpu / max(1, packets) * 1e6, 4),
                          "wall_us_per_packet": round(wall / max(1, packets) * 1e6, 4)}
        finally:
            L.qgcm_tun_close(fd)
    if res["gso"]["packets"] and res["packed"]["packets"]:
        res["cpu_ratio_packed_over_gso"] = round(res["packed"]["cpu_us_per_packet"] / res["gso"]["cpu_us_per_packet"], 3)
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--pipeline-reps", type=int, default=3)
    ap.add_argument("--pipeline-sizes", default="65536,1048576")
    ap.add_argument("--tun-bytes", type=int, default=64 << 20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tun_gso"))
    ap.add_argument("--sections", default="device,pipeline")
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    run = {"device": lambda: device_section(max(20, args.reps)),
           "pipeline": lambda: pipeline_section(max(1, args.pipeline_reps), [int(s) for s in args.pipeline_sizes.split(",")]),
           "tun": lambda: tun_section(args.tun_bytes)}
    for name in args.sections.split(","):
        res = run[name]()
        with open(os.path.join(args.out, f"{name}.json"), "w") as f:
            f.write(json.dumps(res) + "\n")
        print(json.dumps({name: res}), flush=True)


if __name__ == "__main__":
    main()
