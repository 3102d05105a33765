"""ctypes binding of libqgcm.so (include/qgcm.h).

The library is the product: every packet is sealed/opened by the gfx950 kernels inside it.
There is no Python or CPU fallback -- if the shared object is missing or no gfx950 device is
present, loading/creating a context raises.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libqgcm.so")
# tools' A/B runs load another build of the same ABI in its place (never set by the product or the tests)
if os.environ.get("QGCM_AB_LIB"):
    LIB_PATH = os.path.abspath(os.environ["QGCM_AB_LIB"])

# Every symbol include/qgcm.h declares (checked by tests/test_abi.py).
EXPORTS = (
    "qgcm_create", "qgcm_destroy", "qgcm_strerror", "qgcm_version", "qgcm_device_count",
    "qgcm_derive_key", "qgcm_derive_keys", "qgcm_set_key", "qgcm_set_keys", "qgcm_clear_keys",
    "qgcm_x25519_base", "qgcm_x25519",
    "qgcm_derive_keys_device", "qgcm_derive_set_keys", "qgcm_kdf_stats", "qgcm_group_derive_set_keys",
    "qgcm_x25519_batch", "qgcm_x25519_device", "qgcm_peer_keys_device", "qgcm_peers_set_keys", "qgcm_ecdh_stats",
    "qgcm_group_peers_set_keys",
    "qgcm_seal_batch", "qgcm_open_batch", "qgcm_seal_uniform", "qgcm_open_uniform",
    "qgcm_seal_one", "qgcm_open_one", "qgcm_seal_host", "qgcm_open_host",
    "qgcm_random_nonces", "qgcm_nonce_fill", "qgcm_nonce_seed", "qgcm_fill_uniform", "qgcm_host_alloc", "qgcm_host_free",
    "qgcm_stream_copy",
    "qgcm_snappy_max_compressed_length", "qgcm_snappy_compress", "qgcm_snappy_uncompressed_length",
    "qgcm_snappy_uncompress", "qgcm_snappy_compress_slots", "qgcm_snappy_uncompress_slots",
    "qgcm_snappy_compress_slots_limit", "qgcm_compress_seal_host", "qgcm_open_uncompress_host",
    "qgcm_snappy_compress_batch", "qgcm_snappy_uncompress_batch", "qgcm_chain_codec",
    "qgcm_udp_socket", "qgcm_udp_queue", "qgcm_udp_port", "qgcm_udp_close", "qgcm_udp_recv_slots",
    "qgcm_udp_send_slots",
    "qgcm_tun_open", "qgcm_tun_up", "qgcm_tun_read_slots", "qgcm_tun_write_slots", "qgcm_tun_close",
    "qgcm_group_create", "qgcm_group_destroy", "qgcm_group_size", "qgcm_group_ctx", "qgcm_group_shard",
    "qgcm_group_set_keys", "qgcm_group_clear_keys", "qgcm_group_seal_host", "qgcm_group_open_host", "qgcm_group_member_cpus",
    "qgcm_group_last_zerocopy", "qgcm_group_last_path", "qgcm_group_order", "qgcm_launch_counts", "qgcm_resident_stop", "qgcm_resident_stats",
    "qgcm_routes_set", "qgcm_resolve_outgoing", "qgcm_resolve_incoming", "qgcm_route_account", "qgcm_route_stats",
    "qgcm_route_seal_host", "qgcm_route_open_host", "qgcm_udp_send_slots_to",
    "qgcm_peer_plugins_set", "qgcm_peer_plugins_get", "qgcm_chain_outgoing", "qgcm_chain_incoming",
    "qgcm_route_account_bytes", "qgcm_route_chain_seal_host", "qgcm_route_chain_open_host",
    "qgcm_send_plan_work", "qgcm_send_plan", "qgcm_send_plan_cpu", "qgcm_send_plan_host", "qgcm_udp_send_plan",
    "qgcm_udp_gro", "qgcm_udp_recv_gro", "qgcm_gro_unpack", "qgcm_gro_unpack_cpu",
    "qgcm_route_open_gro_host", "qgcm_route_chain_open_gro_host",
    "qgcm_deliver_pack_work", "qgcm_deliver_pack", "qgcm_deliver_pack_cpu", "qgcm_tun_write_packed",
    "qgcm_route_chain_open_packed_host", "qgcm_route_chain_open_gro_packed_host",
    "qgcm_train_pack_work", "qgcm_train_pack", "qgcm_train_pack_cpu", "qgcm_udp_send_packed",
    "qgcm_route_chain_seal_packed_host",
    "qgcm_tun_read_packed", "qgcm_frames_resolve", "qgcm_frames_unpack_cpu", "qgcm_route_chain_seal_frames_host",
    "qgcm_gro_resolve",
    "qgcm_tun_open_offload", "qgcm_tun_read_gso", "qgcm_gso_resolve", "qgcm_gso_unpack_cpu",
    "qgcm_route_chain_seal_gso_host",
    "qgcm_deliver_coalesce_work", "qgcm_deliver_coalesce", "qgcm_deliver_coalesce_cpu", "qgcm_tun_write_gso",
    "qgcm_route_chain_open_coalesced_host", "qgcm_route_chain_open_gro_coalesced_host",
    "qgcm_dtls_sessions_set", "qgcm_dtls_sessions_clear", "qgcm_dtls_session_state", "qgcm_dtls_key_block",
    "qgcm_dtls_seal", "qgcm_dtls_open", "qgcm_dtls_number_cpu", "qgcm_dtls_replay_cpu",
    "qgcm_udp_send_dtls", "qgcm_udp_recv_dtls",
)

QGCM_OK = 0
QGCM_E_ARG = -1
QGCM_E_HIP = -2
QGCM_E_KEY = -3
QGCM_E_AUTH = -4
QGCM_E_NOMEM = -5
OVERHEAD = 28
NO_PEER = 0xFFFFFFFF  # QGCM_NO_PEER: a packet no route resolves, an empty route-table entry
TX, RX = 0, 1  # QGCM_TX / QGCM_RX
PLUGIN_COMPRESSION, PLUGIN_ENCRYPTION = 1, 2  # QGCM_PLUGIN_*: per-peer plugin flags, the node's own mask
GSO_PLAIN, GSO_CSUM, GSO_TCP4, GSO_UDP4 = 0, 1, 2, 3  # QGCM_GSO_*: the kinds of a super-frame table entry
GSO_SEGS = 2048  # QGCM_GSO_SEGS: the most slots one entry names
TUN_TSO4, TUN_USO = 1, 2  # QGCM_TUN_*: the offloads qgcm_tun_open_offload asks for
GRO_SEGS = 64  # QGCM_GRO_SEGS: the most datagrams the kernel coalesces into one received buffer


def chain_work(n: int) -> int:
    """QGCM_CHAIN_WORK(n): bytes of work area a chain call of n packets takes (16-B aligned)."""
    return 4 * ((n + 15) & ~15)


QGCM_MAX_AAD = 16384  # longest additional data of a per-packet call (qgcm_seal_one / qgcm_open_one)
ERRLEN = 120
# QGCM_NONCES_GENERATE: as the nonce argument of a batch seal, "draw the nonces on the GPU from the
# context's AES-256-CTR generator and write them into the slots" (include/qgcm.h)
NONCES_GENERATE = 1


class QgcmError(RuntimeError):
    pass


class Desc(C.Structure):
    """qgcm_desc: {offset u64, len u32, key_idx u32} -- 16 bytes."""

    _fields_ = [("offset", C.c_uint64), ("len", C.c_uint32), ("key_idx", C.c_uint32)]


class Route(C.Structure):
    """qgcm_route: {ip u32 (common.IPtoInt), peer u32 (key slot)}."""

    _fields_ = [("ip", C.c_uint32), ("peer", C.c_uint32)]


class RouteNet(C.Structure):
    """qgcm_route_net: {net, mask, gateway, own_ip}, all common.IPtoInt values."""

    _fields_ = [("net", C.c_uint32), ("mask", C.c_uint32), ("gateway", C.c_uint32), ("own_ip", C.c_uint32)]


class PeerAddr(C.Structure):
    """qgcm_peer_addr: {ip u32, port u16, pad u16}, network byte order."""

    _fields_ = [("ip", C.c_uint32), ("port", C.c_uint16), ("pad", C.c_uint16)]


class Train(C.Structure):
    """qgcm_train: {first (an index into the plan's order), count, peer, seg_len} -- 16 bytes."""

    _fields_ = [("first", C.c_uint32), ("count", C.c_uint32), ("peer", C.c_uint32), ("seg_len", C.c_uint32)]


class PlanLimits(C.Structure):
    """qgcm_plan_limits: {max_segs, max_seg_len, max_bytes}; a zero field takes its default (64, 65507, 65507)."""

    _fields_ = [("max_segs", C.c_uint32), ("max_seg_len", C.c_uint32), ("max_bytes", C.c_uint32)]


class GroBuf(C.Structure):
    """qgcm_gro_buf: {off, len, seg_len (0: no UDP_GRO control message), first (slot of the first datagram)} --
    16 bytes."""

    _fields_ = [("off", C.c_uint32), ("len", C.c_uint32), ("seg_len", C.c_uint32), ("first", C.c_uint32)]


class PackRec(C.Structure):
    """qgcm_pack_rec: {off (0xffffffff: the record did not fit), len, slot, peer} -- 16 bytes."""

    _fields_ = [("off", C.c_uint32), ("len", C.c_uint32), ("slot", C.c_uint32), ("peer", C.c_uint32)]


class PTrain(C.Structure):
    """qgcm_ptrain: {off (0xffffffff: the train did not fit, or is void), count, peer, seg_len} -- 16 bytes."""

    _fields_ = [("off", C.c_uint32), ("count", C.c_uint32), ("peer", C.c_uint32), ("seg_len", C.c_uint32)]


class Frame(C.Structure):
    """qgcm_frame: {off (a multiple of 16), len}: packed[off, off + len) belongs to slot i -- 8 bytes."""

    _fields_ = [("off", C.c_uint32), ("len", C.c_uint32)]


class GsoFrame(C.Structure):
    """qgcm_gso_frame: {off, len, first, count, gso_size u16, hdr_len u16, l4_off u16, csum_off u16, kind, reserved}
    -- 32 bytes."""

    _fields_ = [("off", C.c_uint32), ("len", C.c_uint32), ("first", C.c_uint32), ("count", C.c_uint32),
                ("gso_size", C.c_uint16), ("hdr_len", C.c_uint16), ("l4_off", C.c_uint16), ("csum_off", C.c_uint16),
                ("kind", C.c_uint32), ("reserved", C.c_uint32)]


class DtlsKeys(C.Structure):
    """qgcm_dtls_keys: one session's two keys, IVs, epochs, key slots and next sequence number -- 96 bytes."""

    _fields_ = [("write_key", C.c_uint8 * 32), ("read_key", C.c_uint8 * 32), ("write_iv", C.c_uint8 * 4),
                ("read_iv", C.c_uint8 * 4), ("write_epoch", C.c_uint16), ("read_epoch", C.c_uint16),
                ("write_slot", C.c_uint32), ("read_slot", C.c_uint32), ("write_seq", C.c_uint64)]


_lib: C.CDLL | None = None


def _bind(L: C.CDLL) -> None:
    vp, u8p, sz, u32, u64, i32, lng = C.c_void_p, C.c_char_p, C.c_size_t, C.c_uint32, C.c_uint64, C.c_int, C.c_long
    L.qgcm_create.argtypes = [i32, u32, C.c_char_p, i32]
    L.qgcm_create.restype = vp
    L.qgcm_destroy.argtypes = [vp]
    L.qgcm_destroy.restype = None
    L.qgcm_strerror.argtypes = [i32]
    L.qgcm_strerror.restype = C.c_char_p
    L.qgcm_version.restype = C.c_char_p
    L.qgcm_device_count.argtypes = []
    L.qgcm_device_count.restype = i32
    L.qgcm_derive_key.argtypes = [u8p, sz, u8p, sz, u8p]
    L.qgcm_derive_keys.argtypes = [u8p, u8p, u32, u8p]
    L.qgcm_set_key.argtypes = [vp, u32, u8p]
    L.qgcm_set_keys.argtypes = [vp, u32, u32, u8p]
    if hasattr(L, "qgcm_clear_keys"):
        L.qgcm_clear_keys.argtypes = [vp, u32, u32]
    if hasattr(L, "qgcm_derive_set_keys"):  # (older builds loaded by the A/B tools lack the device KDF)
        L.qgcm_derive_keys_device.argtypes = [vp, u8p, u8p, u32, u32, vp]
        L.qgcm_derive_set_keys.argtypes = [vp, u32, u32, u8p, u8p]
        L.qgcm_kdf_stats.argtypes = [vp, vp, i32]
        L.qgcm_group_derive_set_keys.argtypes = [vp, u32, u32, u8p, u8p]
    if hasattr(L, "qgcm_peers_set_keys"):  # (older builds loaded by the A/B tools lack the device ladders)
        L.qgcm_x25519_batch.argtypes = [u8p, u32, u8p, u32, vp]
        L.qgcm_x25519_device.argtypes = [vp, u8p, u32, u8p, u32, vp]
        L.qgcm_peer_keys_device.argtypes = [vp, u8p, u8p, u8p, u8p, u32, vp]
        L.qgcm_peers_set_keys.argtypes = [vp, u32, u32, u8p, u8p, u8p, u8p]
        L.qgcm_ecdh_stats.argtypes = [vp, vp, i32]
        L.qgcm_group_peers_set_keys.argtypes = [vp, u32, u32, u8p, u8p, u8p, u8p]
    L.qgcm_x25519_base.argtypes = [u8p, u8p]
    L.qgcm_x25519.argtypes = [u8p, u8p, u8p]
    L.qgcm_seal_batch.argtypes = [vp, vp, vp, u32, vp, u32, vp, vp]
    L.qgcm_open_batch.argtypes = [vp, vp, vp, u32, u32, vp, vp]
    L.qgcm_seal_uniform.argtypes = [vp, vp, u64, u32, u32, u32, vp, u32, vp, vp]
    L.qgcm_open_uniform.argtypes = [vp, vp, u64, u32, u32, u32, u32, vp, vp]
    L.qgcm_seal_one.argtypes = [vp, u32, vp, lng, vp, u32, vp]
    L.qgcm_seal_one.restype = lng
    L.qgcm_open_one.argtypes = [vp, u32, vp, lng, vp, u32]
    L.qgcm_open_one.restype = lng
    L.qgcm_seal_host.argtypes = [vp, vp, u64, u32, u32, u32, vp, u32, vp]
    L.qgcm_open_host.argtypes = [vp, vp, u64, u32, u32, u32, u32, vp]
    L.qgcm_random_nonces.argtypes = [vp, u32]
    if hasattr(L, "qgcm_nonce_fill"):  # (older builds loaded by the A/B tools lack the nonce generator)
        L.qgcm_nonce_fill.argtypes = [vp, vp, u32, vp]
        L.qgcm_nonce_seed.argtypes = [vp, u8p, u8p]
    L.qgcm_host_alloc.argtypes = [C.c_size_t]
    L.qgcm_host_alloc.restype = vp
    L.qgcm_host_free.argtypes = [vp]
    L.qgcm_host_free.restype = None
    L.qgcm_stream_copy.argtypes = [vp, vp, vp, u64, vp]
    if hasattr(L, "qgcm_launch_counts"):
        L.qgcm_launch_counts.argtypes = [vp, vp, i32]
    if hasattr(L, "qgcm_resident_stop"):
        L.qgcm_resident_stop.argtypes = [vp]
        L.qgcm_resident_stats.argtypes = [vp, vp, i32]
    sz = C.c_size_t
    L.qgcm_snappy_max_compressed_length.argtypes = [sz]
    L.qgcm_snappy_max_compressed_length.restype = sz
    L.qgcm_snappy_compress.argtypes = [vp, sz, vp, sz]
    L.qgcm_snappy_compress.restype = lng
    L.qgcm_snappy_uncompressed_length.argtypes = [vp, sz]
    L.qgcm_snappy_uncompressed_length.restype = lng
    L.qgcm_snappy_uncompress.argtypes = [vp, sz, vp, sz]
    L.qgcm_snappy_uncompress.restype = lng
    L.qgcm_snappy_compress_slots.argtypes = [vp, u64, u32, vp, C.c_int]
    L.qgcm_snappy_uncompress_slots.argtypes = [vp, u64, u32, vp, vp, C.c_int]
    L.qgcm_fill_uniform.argtypes = [vp, u64, u32, u32, u32, u64, vp, u64, vp]
    L.qgcm_snappy_compress_slots_limit.argtypes = [vp, u64, u32, vp, u64, vp, C.c_int]
    L.qgcm_snappy_compress_batch.argtypes = [vp, vp, u64, u32, vp, u32, u32, vp, vp, u32, vp]
    L.qgcm_snappy_uncompress_batch.argtypes = [vp, vp, u64, u32, vp, u32, u32, vp, vp]
    L.qgcm_chain_codec.argtypes = [vp, i32]
    L.qgcm_compress_seal_host.argtypes = [vp, vp, u64, u32, vp, u32, vp, u32, C.c_int, vp]
    L.qgcm_open_uncompress_host.argtypes = [vp, vp, u64, u32, vp, u32, u32, C.c_int, vp]
    L.qgcm_udp_socket.argtypes = [C.c_char_p, C.c_int, C.c_int]
    L.qgcm_udp_queue.argtypes = [C.c_char_p, C.c_int, C.c_int]
    L.qgcm_udp_port.argtypes = [C.c_int]
    L.qgcm_udp_close.argtypes = [C.c_int]
    L.qgcm_udp_recv_slots.argtypes = [C.c_int, vp, u64, u32, vp, C.c_int]
    L.qgcm_udp_send_slots.argtypes = [C.c_int, vp, u64, u32, vp, C.c_char_p, C.c_int]
    if hasattr(L, "qgcm_group_create"):  # (older builds loaded by the A/B tools lack the group calls)
        L.qgcm_group_create.argtypes = [vp, i32, u32, C.c_char_p, i32]
        L.qgcm_group_create.restype = vp
        L.qgcm_group_destroy.argtypes = [vp]
        L.qgcm_group_destroy.restype = None
        L.qgcm_group_size.argtypes = [vp]
        L.qgcm_group_ctx.argtypes = [vp, i32]
        L.qgcm_group_ctx.restype = vp
        L.qgcm_group_shard.argtypes = [vp, u32]
        L.qgcm_group_set_keys.argtypes = [vp, u32, u32, u8p]
        if hasattr(L, "qgcm_group_clear_keys"):
            L.qgcm_group_clear_keys.argtypes = [vp, u32, u32]
        L.qgcm_group_seal_host.argtypes = [vp, vp, vp, u32, vp, u32, vp]
        L.qgcm_group_open_host.argtypes = [vp, vp, vp, u32, u32, vp]
        if hasattr(L, "qgcm_group_member_cpus"):
            L.qgcm_group_member_cpus.argtypes = [vp, i32]
        if hasattr(L, "qgcm_group_last_zerocopy"):
            L.qgcm_group_last_zerocopy.argtypes = [vp]
        if hasattr(L, "qgcm_group_last_path"):
            L.qgcm_group_last_path.argtypes = [vp, i32]
            L.qgcm_group_order.argtypes = [vp, vp, u32, vp, vp]
    if hasattr(L, "qgcm_routes_set"):  # (older builds loaded by the A/B tools lack the router)
        L.qgcm_routes_set.argtypes = [vp, vp, u32, vp]
        L.qgcm_resolve_outgoing.argtypes = [vp, vp, u64, u32, vp, vp, vp, vp]
        L.qgcm_resolve_incoming.argtypes = [vp, vp, u64, u32, vp, vp, vp, vp]
        L.qgcm_route_account.argtypes = [vp, i32, u32, vp, vp, vp, vp]
        L.qgcm_route_stats.argtypes = [vp, i32, u32, vp]
        L.qgcm_route_seal_host.argtypes = [vp, vp, u64, u32, vp, vp, vp, vp]
        L.qgcm_route_open_host.argtypes = [vp, vp, u64, u32, vp, vp, vp]
        L.qgcm_udp_send_slots_to.argtypes = [C.c_int, vp, u64, u32, vp, vp, vp, u32]
    if hasattr(L, "qgcm_chain_outgoing"):  # (older builds loaded by the A/B tools lack the plugin chain)
        L.qgcm_peer_plugins_set.argtypes = [vp, u32, u32, vp]
        L.qgcm_peer_plugins_get.argtypes = [vp, u32, u32, vp]
        L.qgcm_chain_outgoing.argtypes = [vp, vp, u64, u32, vp, vp, vp, u32, vp, vp, vp, vp, vp]
        L.qgcm_chain_incoming.argtypes = [vp, vp, u64, u32, vp, vp, vp, u32, vp, vp, vp, vp]
        L.qgcm_route_account_bytes.argtypes = [vp, i32, u32, vp, vp, vp, vp]
        L.qgcm_route_chain_seal_host.argtypes = [vp, vp, u64, u32, vp, vp, u32, vp, vp]
        L.qgcm_route_chain_open_host.argtypes = [vp, vp, u64, u32, vp, u32, vp, vp]
    if hasattr(L, "qgcm_send_plan"):  # (older builds loaded by the A/B tools lack the send plan)
        L.qgcm_send_plan_work.argtypes = [u32]
        L.qgcm_send_plan_work.restype = u64
        L.qgcm_send_plan.argtypes = [vp, u32, vp, vp, vp, vp, vp, vp, vp, vp]
        L.qgcm_send_plan_cpu.argtypes = [u32, vp, vp, u32, vp, vp, vp, vp]
        L.qgcm_send_plan_host.argtypes = [vp, u32, vp, vp, vp, vp, vp, vp]
        L.qgcm_udp_send_plan.argtypes = [C.c_int, vp, u64, u32, vp, vp, u32, vp, u32, vp, u32, vp]
    if hasattr(L, "qgcm_gro_unpack"):  # (older builds loaded by the A/B tools lack the coalesced receive)
        L.qgcm_udp_gro.argtypes = [C.c_int, C.c_int]
        L.qgcm_udp_recv_gro.argtypes = [C.c_int, vp, u64, vp, u32, u32, C.c_int, vp]
        L.qgcm_gro_unpack.argtypes = [vp, vp, u64, vp, u32, u32, vp, u64, vp, vp]
        L.qgcm_gro_unpack_cpu.argtypes = [vp, u64, vp, u32, u32, vp, u64, vp]
        L.qgcm_route_open_gro_host.argtypes = [vp, vp, u64, vp, u32, vp, u64, u32, vp, vp, vp]
        L.qgcm_route_chain_open_gro_host.argtypes = [vp, vp, u64, vp, u32, vp, u64, u32, vp, u32, vp, vp]
    if hasattr(L, "qgcm_deliver_pack"):  # (older builds loaded by the A/B tools lack the delivered-packet pack)
        L.qgcm_deliver_pack_work.argtypes = [u32]
        L.qgcm_deliver_pack_work.restype = u64
        L.qgcm_deliver_pack.argtypes = [vp, vp, u64, u32, vp, vp, vp, vp, u64, vp, vp, vp, vp]
        L.qgcm_deliver_pack_cpu.argtypes = [vp, u64, u32, vp, vp, vp, vp, u64, vp, vp]
        L.qgcm_tun_write_packed.argtypes = [C.c_int, vp, u64, vp, u32]
        L.qgcm_route_chain_open_packed_host.argtypes = [vp, vp, u64, u32, vp, u32, vp, vp, vp, u64, vp, vp]
        L.qgcm_route_chain_open_gro_packed_host.argtypes = [vp, vp, u64, vp, u32, u64, u32, vp, u32, vp, vp, vp, u64, vp, vp]
    if hasattr(L, "qgcm_train_pack"):  # (older builds loaded by the A/B tools lack the train pack)
        L.qgcm_train_pack_work.argtypes = [u32]
        L.qgcm_train_pack_work.restype = u64
        L.qgcm_train_pack.argtypes = [vp, vp, u64, u32, vp, vp, vp, vp, u64, vp, vp, vp, vp]
        L.qgcm_train_pack_cpu.argtypes = [vp, u64, u32, vp, u32, vp, u32, vp, u64, vp, vp]
        L.qgcm_udp_send_packed.argtypes = [C.c_int, vp, u64, vp, u32, vp, u32, vp]
        L.qgcm_route_chain_seal_packed_host.argtypes = [vp, vp, u64, u32, vp, vp, u32, vp, vp, vp, vp, u64, vp, vp, vp]
    if hasattr(L, "qgcm_frames_resolve"):  # (older builds loaded by the A/B tools lack the packed frames)
        L.qgcm_tun_read_packed.argtypes = [C.c_int, vp, u64, vp, u32, C.c_int, vp]
        L.qgcm_frames_resolve.argtypes = [vp, vp, u64, vp, u32, vp, u64, vp, vp, vp, vp]
        L.qgcm_frames_unpack_cpu.argtypes = [vp, u64, vp, u32, vp, u64, vp]
        L.qgcm_route_chain_seal_frames_host.argtypes = [vp, vp, u64, vp, u64, u32, vp, vp, u32, vp, vp, vp, vp, u64, vp, vp, vp]
    if hasattr(L, "qgcm_gro_resolve"):  # (older builds loaded by the A/B tools lack the fused receive)
        L.qgcm_gro_resolve.argtypes = [vp, vp, u64, vp, u32, u32, vp, u64, vp, vp, vp, vp]
    if hasattr(L, "qgcm_gso_resolve"):  # (older builds loaded by the A/B tools lack the super-frames)
        L.qgcm_tun_open_offload.argtypes = [C.c_char_p, C.c_int, vp, C.c_char_p, sz, u32]
        L.qgcm_tun_read_gso.argtypes = [C.c_int, vp, u64, vp, u32, u32, C.c_int, vp]
        L.qgcm_gso_resolve.argtypes = [vp, vp, u64, vp, u32, u32, vp, u64, vp, vp, vp, vp]
        L.qgcm_gso_unpack_cpu.argtypes = [vp, u64, vp, u32, u32, vp, u64, vp]
        L.qgcm_route_chain_seal_gso_host.argtypes = [vp, vp, u64, vp, u32, u64, u32, vp, vp, u32, vp, vp, vp, vp, u64, vp, vp, vp]
    if hasattr(L, "qgcm_deliver_coalesce"):  # (older builds loaded by the A/B tools lack the coalescing)
        L.qgcm_deliver_coalesce_work.argtypes = [u32]
        L.qgcm_deliver_coalesce_work.restype = u64
        L.qgcm_deliver_coalesce.argtypes = [vp, vp, u64, u32, vp, vp, vp, vp, u64, vp, vp, vp, vp]
        L.qgcm_deliver_coalesce_cpu.argtypes = [vp, u64, u32, vp, vp, vp, vp, u64, vp, vp]
        L.qgcm_tun_write_gso.argtypes = [C.c_int, vp, u64, vp, u32, vp]
        L.qgcm_route_chain_open_coalesced_host.argtypes = [vp, vp, u64, u32, vp, u32, vp, vp, vp, u64, vp, vp]
        L.qgcm_route_chain_open_gro_coalesced_host.argtypes = [vp, vp, u64, vp, u32, u64, u32, vp, u32, vp, vp, vp, u64, vp, vp]
    if hasattr(L, "qgcm_dtls_seal"):  # (older builds loaded by the A/B tools lack the DTLS record layer)
        L.qgcm_dtls_sessions_set.argtypes = [vp, u32, u32, vp]
        L.qgcm_dtls_sessions_clear.argtypes = [vp, u32, u32]
        L.qgcm_dtls_session_state.argtypes = [vp, u32, vp]
        L.qgcm_dtls_key_block.argtypes = [u8p, u8p, u8p, vp]
        L.qgcm_dtls_seal.argtypes = [vp, vp, u64, u32, vp, vp, vp, vp, vp, vp]
        L.qgcm_dtls_open.argtypes = [vp, vp, u64, u32, vp, vp, vp, vp, vp, vp]
        L.qgcm_dtls_number_cpu.argtypes = [vp, vp, vp, u32, u64, u32, vp, vp, vp, vp, vp]
        L.qgcm_dtls_replay_cpu.argtypes = [u32, vp, vp, vp, u32, vp, vp, i32]
        L.qgcm_udp_send_dtls.argtypes = [C.c_int, vp, u64, u32, vp, vp, vp, vp, vp, u32]
        L.qgcm_udp_recv_dtls.argtypes = [C.c_int, vp, u64, u32, vp, vp, vp, C.c_int, vp]
    if hasattr(L, "qgcm_tun_open"):  # (older builds loaded by the A/B tools lack the TUN calls)
        L.qgcm_tun_open.argtypes = [C.c_char_p, C.c_int, vp, C.c_char_p, sz]
        L.qgcm_tun_up.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int]
        L.qgcm_tun_read_slots.argtypes = [C.c_int, vp, u64, u32, vp, C.c_int]
        L.qgcm_tun_write_slots.argtypes = [C.c_int, vp, u64, u32, vp]
        L.qgcm_tun_close.argtypes = [C.c_int]


def lib() -> C.CDLL:
    """Load libqgcm.so (built in-tree by __graft_entry__.build())."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise QgcmError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
        # Share torch's HIP runtime (same SONAME libamdhip64.so.7) when torch is present: import it first.
        try:
            import torch  # noqa: F401
        except Exception:  # pragma: no cover - torch is plumbing only
            pass
        L = C.CDLL(LIB_PATH)
        _bind(L)
        _lib = L
    return _lib


def check(rc: int, what: str) -> int:
    if rc < 0:
        raise QgcmError(f"{what}: {lib().qgcm_strerror(rc).decode()} ({rc})")
    return rc
