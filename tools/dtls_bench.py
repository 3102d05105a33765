"""DTLS record layer on the device: qgcm_dtls_seal / qgcm_dtls_open against the keyed qgcm_seal_batch /
qgcm_open_batch on the same packets (same count, payload length, number of keys), alternating in one process,
device-event times per call.  Every round seals fresh records (the numbering goes on, so each round's records lie
ahead of the sessions' windows) and opens them: all delivered, checked.

    python tools/dtls_bench.py [--out profiles/dtls/dtls_bench.json] [--rounds 7] [--sizes 4096,65536,262144]

One JSON line per (packets, sessions) to stdout and the file.  No number is a gate."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0  # us


def summary(v):
    return {"median_us": round(statistics.median(v), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/dtls/dtls_bench.json")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sizes", default="4096,65536,262144")
    ap.add_argument("--len", type=int, default=1350)
    args = ap.parse_args()
    import torch

    from quantum_amd import batch, dtls
    from quantum_amd.crypto import Context

    assert torch.cuda.is_available(), "dtls_bench needs the GPU"
    L, stride = args.len, 1536
    rng = np.random.default_rng(0xD7152000)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    lines = []
    for sessions in (1, 64):
        ctx = Context(device=0, max_keys=4 * 64)
        kb = rng.integers(0, 256, (sessions, 72), dtype=np.uint8)
        # session p seals with slot 2p and opens with 2p + 1; session 64 + p is its mirror
        tx = [dtls.Session(kb[p, 0:32].tobytes(), kb[p, 32:64].tobytes(), kb[p, 64:68].tobytes(),
                           kb[p, 68:72].tobytes(), 2 * p, 2 * p + 1) for p in range(sessions)]
        dtls.sessions_set(ctx, 0, tx)
        dtls.sessions_set(ctx, 64, [s.mirrored(128 + 2 * p, 128 + 2 * p + 1) for p, s in enumerate(tx)])
        for n in (int(x) for x in args.sizes.split(",")):
            plain = torch.from_numpy(rng.integers(0, 256, n * stride, dtype=np.uint8)).cuda()
            arena = plain.clone()
            peer_np = (np.arange(n) * 7 % sessions).astype(np.int32)
            peer_tx = torch.from_numpy(peer_np).cuda()
            peer_rx = torch.from_numpy(peer_np + 64).cuda()
            lens0 = torch.full((n,), L, dtype=torch.int32, device="cuda")
            lens = lens0.clone()
            hdr = torch.zeros(32 * n, dtype=torch.uint8, device="cuda")
            status = torch.zeros(n, dtype=torch.uint8, device="cuda")
            # the keyed batch calls on the same packets: [4 B additional data][payload] -> ... [tag][nonce]
            offs = np.arange(n, dtype=np.uint64) * stride
            d_seal = batch.make_descs(offs, np.full(n, L, np.uint32), peer_np.astype(np.uint32) * 2, "cuda")
            d_open = batch.make_descs(offs, np.full(n, L + 28, np.uint32), peer_np.astype(np.uint32) * 2, "cuda")
            nonces = torch.from_numpy(rng.integers(0, 256, 12 * n, dtype=np.uint8)).cuda()
            arena_b = plain.clone()
            t = {"dtls_seal": [], "dtls_open": [], "seal_batch": [], "open_batch": []}
            for r in range(args.rounds + 2):
                arena.copy_(plain)
                lens.copy_(lens0)
                torch.cuda.synchronize()
                a = timed(lambda: dtls.seal(ctx, arena, stride, n, lens, peer_tx, hdr, status))
                assert int(status.sum()) == n
                b = timed(lambda: dtls.open(ctx, arena, stride, n, lens, peer_rx, hdr, status))
                assert int(status.sum()) == n and torch.equal(lens, lens0)
                assert torch.equal(arena.view(n, stride)[:, :L], plain.view(n, stride)[:, :L])
                c = timed(lambda: batch.seal_batch(ctx, arena_b, d_seal, n, nonces, status=status))
                d = timed(lambda: batch.open_batch(ctx, arena_b, d_open, n, status=status))
                assert int(status.sum()) == n
                if r >= 2:
                    for k, v in zip(t, (a, b, c, d)):
                        t[k].append(v)
            line = {"packets": n, "sessions": sessions, "payload": L, "stride": stride, "rounds": args.rounds,
                    **{k: summary(v) for k, v in t.items()}}
            line["payload_gib_s"] = {k: round(n * L / 2 ** 30 / (statistics.median(v) * 1e-6), 1) for k, v in t.items()}
            print(json.dumps(line), flush=True)
            lines.append(line)
        ctx.close()
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
