"""What do GPU-generated nonces cost?  ("Nonces drawn on the GPU".)  Three A/Bs in one
process, the two sides alternating round by round after a warm-up, with bench.py's clock telemetry around
each:

  gen      2^20 nonces: qgcm_random_nonces on the host (wall clock; and the H2D copy of the 12 MiB that
           follows it, device events) against qgcm_nonce_fill on the device (device events)
  uniform  qgcm_seal_uniform of 2^20 x 1350 B (stride 1408, the headline layout) with a resident d_nonces
           array against QGCM_NONCES_GENERATE (device events around the call)
  host     qgcm_seal_host of 64, 1024 and 262144 packets x 1350 B in a pinned arena (stride 1392):
           qgcm_random_nonces + h_nonces (pinned) against QGCM_NONCES_GENERATE (wall clock; the call is
           synchronous)

Prints one JSON line per measurement: median, min and max over the rounds, in microseconds.

    python3 tools/exp_nonce_gen.py [rounds]      (EXP_PARTS="gen,uniform,host")
"""
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from quantum_amd import _lib, batch  # noqa: E402
from quantum_amd.crypto import Context  # noqa: E402


def stats(us: list) -> dict:
    return {"median_us": round(statistics.median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2),
            "rounds": len(us)}


def event_us(fn) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def wall_us(fn) -> float:
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e6


def ab(name: str, sides: dict, rounds: int, warmup: int, extra: dict) -> None:
    """sides: label -> callable returning microseconds; alternated within each round."""
    for _ in range(warmup):
        for fn in sides.values():
            fn()
    tel = bench.GpuTelemetry(0)
    tel.start()
    got = {k: [] for k in sides}
    for _ in range(rounds):
        for k, fn in sides.items():
            got[k].append(fn())
    torch.cuda.synchronize()
    tel.stop()
    clock = tel.summary()
    print(json.dumps({"measurement": name, **extra, **{k: stats(v) for k, v in got.items()},
                      "sclk_mhz_mean": clock["sclk_mhz_mean"], "power_w_mean": clock["power_w_mean"],
                      "telemetry": clock.get("telemetry")}), flush=True)


def main() -> None:
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    parts = os.environ.get("EXP_PARTS", "gen,uniform,host").split(",")
    L = _lib.lib()
    key = bench.derive_key(bench.SECRET, bench.SALT)
    ctx = Context(device=0, max_keys=4)
    ctx.set_key(0, key)
    N, plen = 1 << 20, 1350

    if "gen" in parts:
        h_pageable = np.zeros(12 * N, np.uint8)
        hp = L.qgcm_host_alloc(12 * N)
        h_pinned = np.frombuffer((C.c_uint8 * (12 * N)).from_address(hp), np.uint8)
        d = torch.zeros(12 * N, dtype=torch.uint8, device="cuda")
        pinned_t = torch.from_numpy(h_pinned)
        ab("generate_2^20_nonces", {
            "host_getrandom_pageable": lambda: wall_us(lambda: L.qgcm_random_nonces(h_pageable.ctypes.data, N)),
            "host_getrandom_pinned": lambda: wall_us(lambda: L.qgcm_random_nonces(hp, N)),
            "h2d_copy_12MiB_pinned": lambda: event_us(lambda: d.copy_(pinned_t, non_blocking=True)),
            "device_nonce_fill": lambda: event_us(lambda: batch.nonce_fill(ctx, d, N)),
        }, rounds, 5, {"n": N})
        del pinned_t, h_pinned
        L.qgcm_host_free(hp)

    if "uniform" in parts:
        stride = batch.slot_stride(plen, align=64)
        arena = torch.zeros(N * stride, dtype=torch.uint8, device="cuda")
        nonces = torch.zeros(12 * N, dtype=torch.uint8, device="cuda")
        status = torch.zeros(N, dtype=torch.uint8, device="cuda")
        batch.fill_uniform(arena, stride, N, plen, int.from_bytes(bench.AAD, "little"), 0x5EED0001, nonces, 0x5EED0002)
        ab("seal_uniform_2^20x1350", {
            "resident_d_nonces": lambda: event_us(
                lambda: batch.seal_uniform(ctx, arena, stride, N, plen, 0, nonces, status=status)),
            "generate": lambda: event_us(
                lambda: batch.seal_uniform(ctx, arena, stride, N, plen, 0, batch.GENERATE, status=status)),
        }, rounds, 5, {"n": N, "len": plen, "stride": stride})
        assert int(status.sum()) == N
        del arena, nonces, status

    if "host" in parts:
        stride = 1392
        for n in (64, 1024, 262144):
            ap, npn = L.qgcm_host_alloc(n * stride), L.qgcm_host_alloc(12 * n)
            arena = np.frombuffer((C.c_uint8 * (n * stride)).from_address(ap), np.uint8)
            arena[:] = np.random.default_rng(n).integers(0, 256, n * stride, dtype=np.uint8)
            status = np.zeros(n, np.uint8)

            def with_array():
                L.qgcm_random_nonces(npn, n)
                assert batch.seal_host(ctx, ap, stride, n, plen, 0, npn, status_ptr=status.ctypes.data) == 0

            def generate():
                assert batch.seal_host(ctx, ap, stride, n, plen, 0, batch.GENERATE, status_ptr=status.ctypes.data) == 0

            r = rounds if n > 65536 else max(rounds, 200)
            ab("seal_host_x1350", {"random_nonces_then_h_nonces": lambda: wall_us(with_array),
                                   "generate": lambda: wall_us(generate)}, r, 10, {"n": n, "stride": stride})
            del arena
            L.qgcm_host_free(ap)
            L.qgcm_host_free(npn)
    ctx.close()


if __name__ == "__main__":
    main()
