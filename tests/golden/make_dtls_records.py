"""Writes tests/golden/dtls_records.json from one OpenSSL DTLS 1.2 session (tests/cpp_dtls/ossl_dtls_peer.c, needs
libssl): the session's key block, and records with their plaintexts --
  client_records   written by OpenSSL's client at lengths 1, 15, 16, 17, 33, 1350 and 4081 (23 records)
  server_records   written by OpenSSL's server (the short lengths and 1350)
  model_records    sealed by tests/dtls_model.py with the server's write key (explicit nonce = epoch | seq), each
                   one checked here to come back from the client's SSL_read
so that the GPU tests open what OpenSSL wrote without libssl.  Run from the repository root:
    python tests/golden/make_dtls_records.py"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import dtls_model as M  # noqa: E402
import dtls_peer  # noqa: E402


def plaintext(k: int, L: int) -> bytes:
    return bytes((37 * k + 11 * j + (j >> 8)) & 0xFF for j in range(L))


def main() -> None:
    with tempfile.TemporaryDirectory() as tmp:
        peer = dtls_peer.Peer(dtls_peer.build(tmp))
        block = M.key_block(peer.master, peer.client_random, peer.server_random)
        out = {"cipher": peer.cipher, "epoch": 1, "master": peer.master.hex(),
               "client_random": peer.client_random.hex(), "server_random": peer.server_random.hex(),
               "key_block": block.hex(), "client_records": [], "server_records": [], "model_records": []}
        short = (1, 15, 16, 17, 33)
        for k, L in enumerate(short * 4 + (1350, 1350, 4081)):
            pt = plaintext(k, L)
            out["client_records"].append({"plaintext": pt.hex(), "record": peer.write("c", pt).hex()})
        for k, L in enumerate(short + (1350,)):
            pt = plaintext(100 + k, L)
            out["server_records"].append({"plaintext": pt.hex(), "record": peer.write("s", pt).hex()})
        skey, siv = block[32:64], block[68:72]
        for k, L in enumerate(short + (1350,)):
            pt = plaintext(200 + k, L)
            h = M.header(1, 5000 + k, L)
            rec = h + M.seal_record(skey, siv, h, pt)
            peer.inject("c", rec)
            assert peer.read("c") == pt, "OpenSSL did not take the model's record"
            out["model_records"].append({"plaintext": pt.hex(), "record": rec.hex()})
        peer.close()
    path = os.path.join(HERE, "dtls_records.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
