#!/usr/bin/env python3
"""Peer keys derived on the GPU against the host pool (DESIGN.md "Peer keys derived on the GPU").

    python tools/exp_kdf.py [--out FILE] [--counts 64,256,...] [--no-group]

The driver runs one child process per count (and one for the group step), each under its own `timeout`,
and stops at the first child that fails.  A child makes one timed step per measurement -- the
derivations are far longer than timer noise -- and prints one JSON line:

  host_s        qgcm_derive_keys wall time (its pool is min(hardware_concurrency, 64, count) threads,
                whatever CPU share the process has: `host_threads`, next to `cpus` = the share)
  device_s      qgcm_derive_keys_device wall time (copies in, kernel(s), copy out)
  kernel_ms     the kernel(s) alone, by HIP events on a stream around launch_kdf (the library's internal
                launcher, called by its C++ symbol)
  e2e_device_s  qgcm_derive_set_keys on a context created with QGCM_KDF_DEVICE_MIN=1
  e2e_host_s    qgcm_derive_keys + qgcm_set_keys on a second context
  same          the device keys equal the host keys

The group step (two members on device 0, 1024 keys): install passes per member and wall time of
qgcm_group_set_keys (keys derived on the host first: `derive_s` + `set_s`) against
qgcm_group_derive_set_keys (`derive_set_s`)."""
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

COUNTS = (64, 256, 1024, 4096, 16384, 65536)
LAUNCH_KDF = "_ZN4qgcm10launch_kdfEPKhS1_jjPhP12ihipStream_tPj"  # qgcm::launch_kdf (gcm_internal.h)


def cpu_share() -> int:
    return len(os.sched_getaffinity(0))


def step_count(n: int) -> dict:
    import torch

    from quantum_amd import _lib, crypto

    L = _lib.lib()
    secrets, salts = os.urandom(32 * n), os.urandom(32 * n)
    os.environ["QGCM_KDF_DEVICE_MIN"] = "1"
    dev = crypto.Context(device=0, max_keys=max(n, 2))
    os.environ.pop("QGCM_KDF_DEVICE_MIN")
    host = crypto.Context(device=0, max_keys=max(n, 2))
    crypto.derive_keys_device(dev, secrets[:64], salts[:64], 2)  # the stream and the code object, untimed
    out = {"count": n, "cpus": cpu_share(), "host_threads": min(os.cpu_count() or 1, 64, n)}
    t = time.perf_counter()
    hkeys = crypto.derive_keys(secrets, salts)
    out["host_s"] = time.perf_counter() - t
    t = time.perf_counter()
    dkeys = crypto.derive_keys_device(dev, secrets, salts)
    out["device_s"] = time.perf_counter() - t
    out["same"] = hkeys == dkeys
    # the kernel(s) alone
    launch = getattr(L, LAUNCH_KDF)
    launch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    d_s = torch.frombuffer(bytearray(secrets), dtype=torch.uint8).cuda()
    d_c = torch.frombuffer(bytearray(salts), dtype=torch.uint8).cuda()
    d_k = torch.zeros(32 * n, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    nl = C.c_uint32(0)
    torch.cuda.synchronize()
    e0.record(stream)
    rc = launch(d_s.data_ptr(), d_c.data_ptr(), n, 10000, d_k.data_ptr(), stream.cuda_stream, C.byref(nl))
    e1.record(stream)
    torch.cuda.synchronize()
    out["kernel_ms"] = e0.elapsed_time(e1) if rc == 0 else None
    out["kernel_launches"] = nl.value
    out["same"] = out["same"] and bytes(d_k.cpu().numpy()) == hkeys
    # end to end
    t = time.perf_counter()
    dev.derive_set_keys(0, secrets, salts)
    out["e2e_device_s"] = time.perf_counter() - t
    t = time.perf_counter()
    host.set_keys(0, crypto.derive_keys(secrets, salts))
    out["e2e_host_s"] = time.perf_counter() - t
    out["dev_stats"], out["host_stats"] = dev.kdf_stats(), host.kdf_stats()
    dev.close()
    host.close()
    return out


def step_group(n: int = 1024) -> dict:
    from quantum_amd import crypto, shard

    secrets, salts = os.urandom(32 * n), os.urandom(32 * n)
    out = {"group": 2, "count": n, "cpus": cpu_share()}
    os.environ.pop("QGCM_KDF_DEVICE_MIN", None)
    old = shard.Group([0, 0], max_keys=n)
    t = time.perf_counter()
    keys = crypto.derive_keys(secrets, salts)
    out["derive_s"] = time.perf_counter() - t
    t = time.perf_counter()
    old.set_keys(0, keys)
    out["set_s"] = time.perf_counter() - t
    out["old_passes"] = [old.member(m).kdf_stats()["install_passes"] for m in (0, 1)]
    old.close()
    os.environ["QGCM_KDF_DEVICE_MIN"] = "1"
    new = shard.Group([0, 0], max_keys=n)
    t = time.perf_counter()
    new.derive_set_keys(0, secrets, salts)
    out["derive_set_s"] = time.perf_counter() - t
    st = [new.member(m).kdf_stats() for m in (0, 1)]
    out["new_passes"] = [s["install_passes"] for s in st]
    out["new_device_keys"] = [s["device_keys"] for s in st]
    new.close()
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    ap.add_argument("--counts", default=",".join(str(c) for c in COUNTS))
    ap.add_argument("--no-group", action="store_true")
    ap.add_argument("--step", default=None, help="(child) a count, or 'group'")
    a = ap.parse_args()
    if a.step is not None:
        print(json.dumps(step_group() if a.step == "group" else step_count(int(a.step))), flush=True)
        return 0
    steps = [c for c in a.counts.split(",") if c] + ([] if a.no_group else ["group"])
    for s in steps:
        # the host pool's share of a count dominates: ~7 ms of CPU a key, twice (alone and end to end)
        limit = 120 + (0 if s == "group" else int(s) // 400)
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
