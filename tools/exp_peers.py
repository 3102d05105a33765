#!/usr/bin/env python3
"""A peer table keyed from public keys on the GPU against the host paths (DESIGN.md "Peer secrets computed
on the GPU").

    python tools/exp_peers.py [--out FILE] [--counts 64,1024,65536]

The driver runs one child process per count, each under its own `timeout`, and stops at the first child that
fails.  A child makes one timed step per measurement and prints one JSON line:

  ladder_kernel_ms  the ladder kernel(s) alone over 2 * count lanes, by HIP events on a stream around
                    launch_x25519 (the library's internal launcher, called by its C++ symbol)
  peers_set_s       qgcm_peers_set_keys end to end on a context created with QGCM_KDF_DEVICE_MIN=1
  old_ladders_s     the path before this call existed: a Python loop of 2 * count qgcm_x25519 calls ...
  old_set_s         ... then qgcm_derive_set_keys (default threshold) on a second context
  batch_s           qgcm_x25519_batch over the same 2 * count ladders (its pool is min(hardware_concurrency, 64)
                    threads, whatever CPU share the process has: `cpus`)
  host_path_s       qgcm_peers_set_keys on a context created with QGCM_KDF_DEVICE_MIN=0 (counts up to 1024)
  same              ladder kernel, batch call and loop give the same bytes"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COUNTS = (64, 1024, 65536)
# qgcm::launch_x25519 (gcm_internal.h)
LAUNCH_X25519 = "_ZN4qgcm13launch_x25519EPKhjS1_jPhjP12ihipStream_tPj"


def step_count(n: int) -> dict:
    import torch

    from quantum_amd import _lib, crypto

    L = _lib.lib()
    priv_key, priv_salt = os.urandom(32), os.urandom(32)
    nine = bytes([9]) + bytes(31)
    pub_keys = crypto.x25519_batch(os.urandom(32 * n), nine * n)
    pub_salts = crypto.x25519_batch(os.urandom(32 * n), nine * n)
    os.environ["QGCM_KDF_DEVICE_MIN"] = "1"
    dev = crypto.Context(device=0, max_keys=max(n, 2))
    os.environ.pop("QGCM_KDF_DEVICE_MIN")
    old = crypto.Context(device=0, max_keys=max(n, 2))
    crypto.x25519_device(dev, priv_key, pub_keys[:64])  # the stream and the code object, untimed
    crypto.derive_keys_device(dev, pub_keys[:64], pub_salts[:64], 2)
    out = {"count": n, "cpus": len(os.sched_getaffinity(0)), "host_threads": min(os.cpu_count() or 1, 64, 2 * n)}
    # the ladder kernel(s) alone: 2 * count lanes, the two private scalars split at count
    launch = getattr(L, LAUNCH_X25519)
    launch.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    d_k = torch.frombuffer(bytearray(priv_key + priv_salt), dtype=torch.uint8).cuda()
    d_p = torch.frombuffer(bytearray(pub_keys + pub_salts), dtype=torch.uint8).cuda()
    d_o = torch.zeros(64 * n, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    nl = C.c_uint32(0)
    torch.cuda.synchronize()
    e0.record(stream)
    rc = launch(d_k.data_ptr(), 0, d_p.data_ptr(), 2 * n, d_o.data_ptr(), n, stream.cuda_stream, C.byref(nl))
    e1.record(stream)
    torch.cuda.synchronize()
    out["ladder_kernel_ms"] = e0.elapsed_time(e1) if rc == 0 else None
    out["ladder_launches"] = nl.value
    shared_dev = bytes(d_o.cpu().numpy())
    # end to end on the device
    t = time.perf_counter()
    dev.peers_set_keys(0, priv_key, priv_salt, pub_keys, pub_salts)
    out["peers_set_s"] = time.perf_counter() - t
    # the path before: one qgcm_x25519 call per ladder from Python, then qgcm_derive_set_keys
    t = time.perf_counter()
    secrets = b"".join(crypto.x25519(priv_key, pub_keys[i:i + 32]) for i in range(0, 32 * n, 32))
    salts = b"".join(crypto.x25519(priv_salt, pub_salts[i:i + 32]) for i in range(0, 32 * n, 32))
    out["old_ladders_s"] = time.perf_counter() - t
    t = time.perf_counter()
    old.derive_set_keys(0, secrets, salts)
    out["old_set_s"] = time.perf_counter() - t
    # the host pool
    t = time.perf_counter()
    shared_batch = crypto.x25519_batch(priv_key, pub_keys) + crypto.x25519_batch(priv_salt, pub_salts)
    out["batch_s"] = time.perf_counter() - t
    out["same"] = shared_dev == shared_batch == secrets + salts
    if n <= 1024:
        os.environ["QGCM_KDF_DEVICE_MIN"] = "0"
        host = crypto.Context(device=0, max_keys=max(n, 2))
        os.environ.pop("QGCM_KDF_DEVICE_MIN")
        t = time.perf_counter()
        host.peers_set_keys(0, priv_key, priv_salt, pub_keys, pub_salts)
        out["host_path_s"] = time.perf_counter() - t
        host.close()
    out["dev_ecdh"], out["dev_kdf"], out["old_kdf"] = dev.ecdh_stats(), dev.kdf_stats(), old.kdf_stats()
    dev.close()
    old.close()
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    ap.add_argument("--counts", default=",".join(str(c) for c in COUNTS))
    ap.add_argument("--step", default=None, help="(child) a count")
    a = ap.parse_args()
    if a.step is not None:
        print(json.dumps(step_count(int(a.step))), flush=True)
        return 0
    for s in [c for c in a.counts.split(",") if c]:
        # the Python loop of single ladders dominates: ~0.1 ms of one core a ladder, 2 * count of them
        limit = 120 + int(s) // 1000
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", s],
                           capture_output=True, text=True)
        line = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else ""
        if r.returncode != 0 or not line.startswith("{"):
            print(f"step {s}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}", flush=True)
            return 1  # nothing more on the GPU after a failed step
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
