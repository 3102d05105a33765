"""The ABI around long additional data, without a device: QGCM_MAX_AAD is visible through the Python
binding with the header's value, and the batch entry points did not move -- they still take at most the
4-byte IP header and answer QGCM_E_ARG beyond it."""
import ctypes as C
import os
import re

from conftest import ROOT


def header_define(name):
    with open(os.path.join(ROOT, "include", "qgcm.h")) as f:
        m = re.search(rf"^#define\s+{name}\s+(\S+)", f.read(), re.M)
    assert m, f"{name} is not defined in include/qgcm.h"
    return int(m.group(1), 0)


def test_max_aad_matches_the_header():
    from quantum_amd import _lib, crypto

    assert header_define("QGCM_MAX_AAD") == 16384
    assert _lib.QGCM_MAX_AAD == header_define("QGCM_MAX_AAD")
    assert crypto.MaxAdditional == _lib.QGCM_MAX_AAD


def test_batch_calls_still_refuse_more_than_four_bytes():
    from quantum_amd import _lib

    L = C.CDLL(_lib.LIB_PATH)
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    L.qgcm_seal_uniform.argtypes = [vp, vp, u64, u32, u32, u32, vp, u32, vp, vp]
    L.qgcm_seal_batch.argtypes = [vp, vp, vp, u32, vp, u32, vp, vp]
    L.qgcm_seal_host.argtypes = [vp, vp, u64, u32, u32, u32, vp, u32, vp]
    for fn in (L.qgcm_seal_uniform, L.qgcm_seal_batch, L.qgcm_seal_host):
        fn.restype = C.c_int
    assert L.qgcm_seal_uniform(None, None, 1392, 1, 1350, 0, None, 5, None, None) == _lib.QGCM_E_ARG
    assert L.qgcm_seal_batch(None, None, None, 1, None, 5, None, None) == _lib.QGCM_E_ARG
    assert L.qgcm_seal_host(None, None, 1392, 1, 1350, 0, None, 5, None) == _lib.QGCM_E_ARG
