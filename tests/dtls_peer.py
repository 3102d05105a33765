"""The OpenSSL DTLS 1.2 session of tests/cpp_dtls/ossl_dtls_peer.c as a child process: built on demand with the
host compiler, spoken to over stdin / stdout.  Used by tests/test_dtls_openssl.py and
tests/golden/make_dtls_records.py."""
from __future__ import annotations

import ctypes.util
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def available() -> bool:
    """libssl and its headers are installed."""
    return bool(ctypes.util.find_library("ssl")) and os.path.exists("/usr/include/openssl/ssl.h")


def build(out_dir: str) -> str:
    exe = os.path.join(out_dir, "ossl_dtls_peer")
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp_dtls"), "peer", f"PEER={exe}"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


class Peer:
    """One established session: side "c" is the client, "s" the server."""

    def __init__(self, exe: str):
        self.p = subprocess.Popen([exe], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, bufsize=1)
        assert self._line() == "ready"
        self.p.stdin.write("keys\n")
        kv = dict(self._line().split(" ", 1) for _ in range(4))
        self.master = bytes.fromhex(kv["master"])
        self.client_random = bytes.fromhex(kv["client_random"])
        self.server_random = bytes.fromhex(kv["server_random"])
        self.cipher = kv["cipher"]

    def _line(self) -> str:
        line = self.p.stdout.readline()
        assert line, "ossl_dtls_peer ended"
        return line.rstrip("\n")

    def write(self, side: str, plaintext: bytes) -> bytes:
        """SSL_write on `side`; the record it put on the wire, taken off it."""
        self.p.stdin.write(f"{side}write {plaintext.hex()}\n")
        tag, rec = self._line().split(" ", 1)
        assert tag == "record"
        return bytes.fromhex(rec)

    def inject(self, side: str, record: bytes) -> None:
        """A datagram on the wire towards `side`."""
        self.p.stdin.write(f"{side}inject {record.hex()}\n")
        assert self._line() == "ok"

    def read(self, side: str) -> bytes | None:
        """SSL_read on `side`: the plaintext, or None when nothing was deliverable."""
        self.p.stdin.write(f"{side}read\n")
        line = self._line()
        return None if line == "none" else bytes.fromhex(line.split(" ", 1)[1])

    def close(self) -> None:
        if self.p.poll() is None:
            self.p.stdin.write("quit\n")
            self.p.stdin.close()
            self.p.wait(timeout=30)
        self.p.stdout.close()
