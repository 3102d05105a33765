// udp_batch.cpp -- socket/udp.go:35-47 batched.
//
// The reference moves one datagram per syscall: Read = recvfrom into the worker's Raw buffer then
// NewSockPayload(buf, n); Write = sendto(Raw[:Length], mapping.Sockaddr).  A GPU batch of thousands
// of packets needs the I/O batched too, or the path is syscall-bound long before it is crypto-bound.
// These calls move whole batches of Payload.Raw slots (slot i at arena + i*stride; the datagram IS
// Raw[:Length], wire format [4-B private IP][ct][tag][nonce]) with recvmmsg / sendmmsg, straight
// into / out of the (pinned) host arena that qgcm_seal_host / qgcm_open_host and the chained
// snappy paths consume, so the datagram bytes are never copied on the host.
#include <arpa/inet.h>
#include <errno.h>
#include <netinet/in.h>
#include <netinet/udp.h>
#include <poll.h>
#include <stdlib.h>
#include <string.h>
#include <sys/socket.h>
#include <unistd.h>

#include <algorithm>
#include <vector>

#include "../../include/qgcm.h"
#include "coalesce_core.h"
#include "gro_core.h"
#include "pack_core.h"
#include "train_core.h"

#ifndef UDP_SEGMENT
#define UDP_SEGMENT 103  // linux/udp.h, Linux 4.18
#endif
#ifndef UDP_GRO
#define UDP_GRO 104  // linux/udp.h, Linux 5.0
#endif
#ifndef SOL_UDP
#define SOL_UDP 17
#endif

namespace {

constexpr unsigned kVlen = 1024;  // UIO_MAXIOV: most messages one recvmmsg/sendmmsg call takes
constexpr uint64_t kGroRoom = 65536;  // room one coalesced receive needs: no buffer is longer than 65535 bytes

bool make_addr(const char *ip, int port, sockaddr_in *a) {
    memset(a, 0, sizeof *a);
    a->sin_family = AF_INET;
    a->sin_port = htons((uint16_t)port);
    return port >= 0 && port <= 65535 && inet_pton(AF_INET, ip, &a->sin_addr) == 1;
}

}  // namespace

extern "C" {

// socket/udp.go:49-70 (createUDPSocket): one queue.  rcvbuf_bytes > 0 also sizes SO_RCVBUF/SO_SNDBUF
// (a batch of packets must fit the kernel buffer between two recvmmsg calls).
int qgcm_udp_socket(const char *ip, int port, int bufbytes) {
    sockaddr_in a;
    if (!ip || !make_addr(ip, port, &a)) return -1;
    const int fd = socket(AF_INET, SOCK_DGRAM | SOCK_CLOEXEC, 0);
    if (fd < 0) return -1;
    const int one = 1;
    setsockopt(fd, SOL_SOCKET, SO_REUSEADDR, &one, sizeof one);
    if (bufbytes > 0) {
        setsockopt(fd, SOL_SOCKET, SO_RCVBUF, &bufbytes, sizeof bufbytes);
        setsockopt(fd, SOL_SOCKET, SO_SNDBUF, &bufbytes, sizeof bufbytes);
    }
    if (bind(fd, reinterpret_cast<sockaddr *>(&a), sizeof a) != 0) {
        close(fd);
        return -1;
    }
    return fd;
}

// One queue of a multi-queue UDP socket: socket/udp.go:55-70 (newUDP) opens cfg.NumWorkers sockets on
// the same ListenAddr, one per worker (socket.go:52-77 sets SO_REUSEADDR).  On Linux only SO_REUSEPORT
// spreads the incoming datagrams over such a group -- by a hash of the sender's address and port, so
// each flow stays on one queue and in order -- which is what the per-worker queues are for.  Every
// queue of a group must be opened by the same user; a port of 0 is resolved by the first queue
// (qgcm_udp_port) and passed to the others.
int qgcm_udp_queue(const char *ip, int port, int bufbytes) {
    sockaddr_in a;
    if (!ip || !make_addr(ip, port, &a)) return -1;
    const int fd = socket(AF_INET, SOCK_DGRAM | SOCK_CLOEXEC, 0);
    if (fd < 0) return -1;
    const int one = 1;
    if (setsockopt(fd, SOL_SOCKET, SO_REUSEADDR, &one, sizeof one) != 0 ||
        setsockopt(fd, SOL_SOCKET, SO_REUSEPORT, &one, sizeof one) != 0) {
        close(fd);
        return -1;
    }
    if (bufbytes > 0) {
        setsockopt(fd, SOL_SOCKET, SO_RCVBUF, &bufbytes, sizeof bufbytes);
        setsockopt(fd, SOL_SOCKET, SO_SNDBUF, &bufbytes, sizeof bufbytes);
    }
    if (bind(fd, reinterpret_cast<sockaddr *>(&a), sizeof a) != 0) {
        close(fd);
        return -1;
    }
    return fd;
}

int qgcm_udp_port(int fd) {
    sockaddr_in a;
    socklen_t n = sizeof a;
    if (getsockname(fd, reinterpret_cast<sockaddr *>(&a), &n) != 0) return -1;
    return ntohs(a.sin_port);
}

int qgcm_udp_close(int fd) { return close(fd) == 0 ? 0 : -1; }

// socket/udp.go:35-41, batched: waits up to timeout_ms (-1 = forever) for the first datagram, then
// takes every datagram already queued, up to max_n, into slots 0, 1, ... (lens[i] = its length, as
// NewSockPayload(buf, n)).  A datagram longer than the slot is truncated to `stride` bytes, as
// recvfrom into the worker's buffer truncates.  Returns the number received (0 on timeout) or -1.
int qgcm_udp_recv_slots(int fd, uint8_t *arena, uint64_t stride, uint32_t max_n, uint32_t *lens, int timeout_ms) {
    if (fd < 0 || (max_n && (!arena || !lens)) || stride == 0) return -1;
    if (max_n == 0) return 0;
    pollfd p{fd, POLLIN, 0};
    int pr;
    do {
        pr = poll(&p, 1, timeout_ms);
    } while (pr < 0 && errno == EINTR);
    if (pr < 0) return -1;
    if (pr == 0) return 0;
    std::vector<mmsghdr> msgs(std::min<uint32_t>(max_n, kVlen));
    std::vector<iovec> iov(msgs.size());
    uint32_t got = 0;
    while (got < max_n) {
        const unsigned k = (unsigned)std::min<uint64_t>(max_n - got, msgs.size());
        for (unsigned i = 0; i < k; ++i) {
            iov[i] = iovec{arena + (uint64_t)(got + i) * stride, (size_t)stride};
            msgs[i] = mmsghdr{};
            msgs[i].msg_hdr.msg_iov = &iov[i];
            msgs[i].msg_hdr.msg_iovlen = 1;
        }
        const int r = recvmmsg(fd, msgs.data(), k, MSG_DONTWAIT, nullptr);
        if (r < 0) {
            if (errno == EINTR) continue;
            if (errno == EAGAIN || errno == EWOULDBLOCK) break;
            return got ? (int)got : -1;
        }
        for (int i = 0; i < r; ++i) lens[got + i] = msgs[i].msg_len;
        got += (uint32_t)r;
        if ((unsigned)r < k) break;
    }
    return (int)got;
}

// socket/udp.go:43-47, batched: sends Raw[:lens[i]] of slots 0..n-1 to ip:port (one peer's batch,
// mapping.Sockaddr).  Blocks while the socket buffer is full, as sendto does.  Returns the number
// of datagrams sent (n on success) or -1 if none could be.
int qgcm_udp_send_slots(int fd, const uint8_t *arena, uint64_t stride, uint32_t n, const uint32_t *lens,
                        const char *ip, int port) {
    sockaddr_in dst;
    if (fd < 0 || (n && (!arena || !lens)) || !ip || !make_addr(ip, port, &dst)) return -1;
    std::vector<mmsghdr> msgs(std::min<uint32_t>(std::max<uint32_t>(n, 1), kVlen));
    std::vector<iovec> iov(msgs.size());
    uint32_t sent = 0;
    while (sent < n) {
        const unsigned k = (unsigned)std::min<uint64_t>(n - sent, msgs.size());
        for (unsigned i = 0; i < k; ++i) {
            iov[i] = iovec{const_cast<uint8_t *>(arena) + (uint64_t)(sent + i) * stride,
                           (size_t)std::min<uint64_t>(lens[sent + i], stride)};
            msgs[i] = mmsghdr{};
            msgs[i].msg_hdr.msg_name = &dst;
            msgs[i].msg_hdr.msg_namelen = sizeof dst;
            msgs[i].msg_hdr.msg_iov = &iov[i];
            msgs[i].msg_hdr.msg_iovlen = 1;
        }
        const int r = sendmmsg(fd, msgs.data(), k, 0);
        if (r < 0) {
            if (errno == EINTR) continue;
            return sent ? (int)sent : -1;
        }
        sent += (uint32_t)r;
    }
    return (int)sent;
}

// socket/udp.go:43-47 with mapping.Sockaddr per packet: datagram i = Raw[:lens[i]] of slot i goes to
// addrs[peer[i]] (what qgcm_route_seal_host left in h_lens and h_peer).  Packets with peer[i] ==
// QGCM_NO_PEER or lens[i] == 0 (unroutable, or dropped by the seal) are skipped.  A peer[i] at or past
// n_addrs fails the whole call before anything is sent.  Returns the number of datagrams sent, or -1.
int qgcm_udp_send_slots_to(int fd, const uint8_t *arena, uint64_t stride, uint32_t n, const uint32_t *lens,
                           const uint32_t *peer, const qgcm_peer_addr *addrs, uint32_t n_addrs) {
    if (fd < 0 || (n && (!arena || !lens || !peer)) || (n_addrs && !addrs)) return -1;
    for (uint32_t i = 0; i < n; ++i)
        if (peer[i] != QGCM_NO_PEER && lens[i] != 0 && peer[i] >= n_addrs) return -1;
    std::vector<mmsghdr> msgs(kVlen);
    std::vector<iovec> iov(kVlen);
    std::vector<sockaddr_in> dst(kVlen);
    uint32_t next = 0, sent = 0;
    while (next < n) {
        unsigned k = 0;
        for (; next < n && k < kVlen; ++next) {
            if (peer[next] == QGCM_NO_PEER || lens[next] == 0) continue;
            const qgcm_peer_addr &a = addrs[peer[next]];
            memset(&dst[k], 0, sizeof dst[k]);
            dst[k].sin_family = AF_INET;
            dst[k].sin_addr.s_addr = a.ip;  // network byte order already
            dst[k].sin_port = a.port;
            iov[k] = iovec{const_cast<uint8_t *>(arena) + (uint64_t)next * stride,
                           (size_t)std::min<uint64_t>(lens[next], stride)};
            msgs[k] = mmsghdr{};
            msgs[k].msg_hdr.msg_name = &dst[k];
            msgs[k].msg_hdr.msg_namelen = sizeof dst[k];
            msgs[k].msg_hdr.msg_iov = &iov[k];
            msgs[k].msg_hdr.msg_iovlen = 1;
            ++k;
        }
        for (unsigned done = 0; done < k;) {
            const int r = sendmmsg(fd, msgs.data() + done, k - done, 0);
            if (r < 0) {
                if (errno == EINTR) continue;
                return sent ? (int)sent : -1;
            }
            done += (unsigned)r;
            sent += (uint32_t)r;
        }
    }
    return (int)sent;
}

// socket/udp.go:43-47 for a planned batch (qgcm_send_plan*): one message per train, its datagrams gathered
// from their slots by one iovec each, cut apart again by the kernel's UDP_SEGMENT (one traversal of the UDP
// stack per train in place of one per datagram).  The contract is in include/qgcm.h.
int qgcm_udp_send_plan(int fd, const uint8_t *arena, uint64_t stride, uint32_t n, const uint32_t *lens,
                       const uint32_t *order, uint32_t m, const qgcm_train *trains, uint32_t n_trains,
                       const qgcm_peer_addr *addrs, uint32_t n_addrs, uint64_t stats[3]) {
    if (stats) stats[0] = stats[1] = stats[2] = 0;
    if (fd < 0 || (n && (!arena || !lens)) || (m && !order) || (n_trains && !trains) || (n_addrs && !addrs)) return -1;
    // the whole plan before the first byte leaves
    for (uint32_t j = 0; j < m; ++j)
        if (order[j] >= n) return -1;
    for (uint32_t t = 0; t < n_trains; ++t) {
        const qgcm_train &tr = trains[t];
        if (tr.count < 1 || tr.count > kVlen || (uint64_t)tr.first + tr.count > m || tr.peer >= n_addrs) return -1;
        // an empty datagram is never sendable; a segment size travels as 16 bits
        if (tr.seg_len == 0 || tr.seg_len > stride || (tr.count > 1 && tr.seg_len > 65535u)) return -1;
        for (uint32_t k = 0; k < tr.count; ++k)
            if (lens[order[tr.first + k]] != tr.seg_len) return -1;
    }
    const char *gso_env = getenv("QGCM_UDP_GSO");
    bool gso = !(gso_env && !strcmp(gso_env, "0"));

    constexpr unsigned kIovPool = 4 * kVlen;  // a train takes at most kVlen of them
    struct SegCtl {
        alignas(cmsghdr) char buf[CMSG_SPACE(sizeof(uint16_t))];
    };
    std::vector<mmsghdr> msgs(kVlen);
    std::vector<iovec> iov(kIovPool);
    std::vector<sockaddr_in> dst(kVlen);
    std::vector<SegCtl> ctl(kVlen);
    std::vector<uint32_t> msg_train(kVlen);  // the train of each queued message
    uint64_t sent = 0, n_msgs = 0, n_seg = 0, n_fell = 0;
    auto finish = [&](bool failed) {
        if (stats) {
            stats[0] = n_msgs;
            stats[1] = n_seg;
            stats[2] = n_fell;
        }
        return failed && sent == 0 ? -1 : (int)sent;
    };
    auto slot_iov = [&](uint32_t pos, uint32_t len) {
        return iovec{const_cast<uint8_t *>(arena) + (uint64_t)order[pos] * stride, (size_t)len};
    };
    auto set_dst = [&](sockaddr_in *d, uint32_t peer) {
        memset(d, 0, sizeof *d);
        d->sin_family = AF_INET;
        d->sin_addr.s_addr = addrs[peer].ip;  // network byte order already
        d->sin_port = addrs[peer].port;
    };
    // a train as `count` plain datagrams (count <= kVlen), through buffers of its own: the segmented
    // messages queued behind a train that fell back keep theirs; false: a send failed
    std::vector<mmsghdr> one_msgs;
    std::vector<iovec> one_iov;
    sockaddr_in one_dst;
    auto send_singles = [&](const qgcm_train &tr) {
        one_msgs.resize(kVlen);
        one_iov.resize(kVlen);
        set_dst(&one_dst, tr.peer);
        for (uint32_t i = 0; i < tr.count; ++i) {
            one_iov[i] = slot_iov(tr.first + i, tr.seg_len);
            one_msgs[i] = mmsghdr{};
            one_msgs[i].msg_hdr.msg_name = &one_dst;
            one_msgs[i].msg_hdr.msg_namelen = sizeof one_dst;
            one_msgs[i].msg_hdr.msg_iov = &one_iov[i];
            one_msgs[i].msg_hdr.msg_iovlen = 1;
        }
        for (uint32_t done = 0; done < tr.count;) {
            const int r = sendmmsg(fd, one_msgs.data() + done, tr.count - done, 0);
            if (r < 0) {
                if (errno == EINTR) continue;
                return false;
            }
            done += (uint32_t)r;
            sent += (uint64_t)r;
            n_msgs += (uint64_t)r;
        }
        return true;
    };

    uint32_t next = 0;  // the next train to queue
    while (next < n_trains) {
        unsigned k = 0, used = 0;  // messages and iovecs queued; an empty queue takes any train
        for (; next < n_trains; ++next) {
            const qgcm_train &tr = trains[next];
            // a segmented train is one message of `count` iovecs; a train of one, and every train under
            // QGCM_UDP_GSO=0, is `count` plain messages
            const bool seg = gso && tr.count > 1;
            const unsigned n_new = seg ? 1u : tr.count;
            if (k + n_new > kVlen || used + tr.count > kIovPool) break;
            for (uint32_t i = 0; i < tr.count; ++i) iov[used + i] = slot_iov(tr.first + i, tr.seg_len);
            for (unsigned i = 0; i < n_new; ++i, ++k) {
                set_dst(&dst[k], tr.peer);
                msgs[k] = mmsghdr{};
                msghdr &h = msgs[k].msg_hdr;
                h.msg_name = &dst[k];
                h.msg_namelen = sizeof dst[k];
                h.msg_iov = &iov[used + i];
                h.msg_iovlen = seg ? tr.count : 1;
                if (seg) {
                    memset(ctl[k].buf, 0, sizeof ctl[k].buf);
                    h.msg_control = ctl[k].buf;
                    h.msg_controllen = sizeof ctl[k].buf;
                    cmsghdr *cm = CMSG_FIRSTHDR(&h);
                    cm->cmsg_level = SOL_UDP;
                    cm->cmsg_type = UDP_SEGMENT;
                    cm->cmsg_len = CMSG_LEN(sizeof(uint16_t));
                    const uint16_t seg_len = (uint16_t)tr.seg_len;
                    memcpy(CMSG_DATA(cm), &seg_len, sizeof seg_len);
                }
                msg_train[k] = next;
            }
            used += tr.count;
        }
        for (unsigned done = 0; done < k;) {
            const int r = sendmmsg(fd, msgs.data() + done, k - done, 0);
            if (r >= 0) {
                for (int i = 0; i < r; ++i) {  // a message carries one datagram per iovec
                    sent += msgs[done + i].msg_hdr.msg_iovlen;
                    n_seg += msgs[done + i].msg_hdr.msg_iovlen > 1;
                }
                n_msgs += (uint64_t)r;
                done += (unsigned)r;
                continue;
            }
            if (errno == EINTR) continue;
            // msgs[done] is the one that failed
            const bool unsupported = errno == ENOPROTOOPT || errno == EOPNOTSUPP;
            const bool refused = unsupported || errno == EINVAL || errno == EIO || errno == EMSGSIZE;
            if (msgs[done].msg_hdr.msg_iovlen == 1 || !refused) return finish(true);
            ++n_fell;
            if (!send_singles(trains[msg_train[done]])) return finish(true);
            ++done;
            if (unsupported) {
                // this socket takes no UDP_SEGMENT at all: the trains queued behind this one, and the rest
                // of the call, go unsegmented without asking again
                gso = false;
                if (done < k) next = msg_train[done];
                break;
            }
        }
    }
    return finish(false);
}

// socket/udp.go:43-47 for a planned batch whose trains the GPU has packed (qgcm_train_pack, or
// qgcm_route_chain_seal_packed_host): qgcm_udp_send_plan with every train one contiguous stretch of the packed
// area, so a message is one iovec whatever its count.  The contract is in include/qgcm.h.
int qgcm_udp_send_packed(int fd, const uint8_t *packed, uint64_t packed_len, const qgcm_ptrain *ptrains,
                         uint32_t n_trains, const qgcm_peer_addr *addrs, uint32_t n_addrs, uint64_t stats[3]) {
    if (stats) stats[0] = stats[1] = stats[2] = 0;
    if (fd < 0 || (n_trains && (!packed || !ptrains)) || (n_addrs && !addrs)) return -1;
    // the whole table before the first byte leaves
    if (!qgcm::train_table_ok(ptrains, n_trains, packed_len, n_addrs)) return -1;
    const char *gso_env = getenv("QGCM_UDP_GSO");
    bool gso = !(gso_env && !strcmp(gso_env, "0"));

    struct SegCtl {
        alignas(cmsghdr) char buf[CMSG_SPACE(sizeof(uint16_t))];
    };
    std::vector<mmsghdr> msgs(kVlen);
    std::vector<iovec> iov(kVlen);  // one a message
    std::vector<sockaddr_in> dst(kVlen);
    std::vector<SegCtl> ctl(kVlen);
    std::vector<uint32_t> msg_train(kVlen);  // the train of each queued message
    std::vector<uint32_t> msg_dgrams(kVlen); // the datagrams it carries
    uint64_t sent = 0, n_msgs = 0, n_seg = 0, n_fell = 0;
    auto finish = [&](bool failed) {
        if (stats) {
            stats[0] = n_msgs;
            stats[1] = n_seg;
            stats[2] = n_fell;
        }
        return failed && sent == 0 ? -1 : (int)sent;
    };
    // datagram i of a train, cut from the packed bytes
    auto cut_iov = [&](const qgcm_ptrain &tr, uint32_t i, uint32_t count) {
        return iovec{const_cast<uint8_t *>(packed) + tr.off + (uint64_t)i * tr.seg_len, (size_t)count * tr.seg_len};
    };
    auto set_dst = [&](sockaddr_in *d, uint32_t peer) {
        memset(d, 0, sizeof *d);
        d->sin_family = AF_INET;
        d->sin_addr.s_addr = addrs[peer].ip;  // network byte order already
        d->sin_port = addrs[peer].port;
    };
    // a train as `count` plain datagrams (count <= kVlen), through buffers of its own: the segmented
    // messages queued behind a train that fell back keep theirs; false: a send failed
    std::vector<mmsghdr> one_msgs;
    std::vector<iovec> one_iov;
    sockaddr_in one_dst;
    auto send_singles = [&](const qgcm_ptrain &tr) {
        one_msgs.resize(kVlen);
        one_iov.resize(kVlen);
        set_dst(&one_dst, tr.peer);
        for (uint32_t i = 0; i < tr.count; ++i) {
            one_iov[i] = cut_iov(tr, i, 1);
            one_msgs[i] = mmsghdr{};
            one_msgs[i].msg_hdr.msg_name = &one_dst;
            one_msgs[i].msg_hdr.msg_namelen = sizeof one_dst;
            one_msgs[i].msg_hdr.msg_iov = &one_iov[i];
            one_msgs[i].msg_hdr.msg_iovlen = 1;
        }
        for (uint32_t done = 0; done < tr.count;) {
            const int r = sendmmsg(fd, one_msgs.data() + done, tr.count - done, 0);
            if (r < 0) {
                if (errno == EINTR) continue;
                return false;
            }
            done += (uint32_t)r;
            sent += (uint64_t)r;
            n_msgs += (uint64_t)r;
        }
        return true;
    };

    uint32_t next = 0;  // the next train to queue
    while (next < n_trains) {
        unsigned k = 0;  // messages queued; an empty queue takes any train
        for (; next < n_trains; ++next) {
            const qgcm_ptrain &tr = ptrains[next];
            // a segmented train is one message over the train's bytes; a train of one, and every train under
            // QGCM_UDP_GSO=0, is `count` plain messages
            const bool seg = gso && tr.count > 1;
            const unsigned n_new = seg ? 1u : tr.count;
            if (k + n_new > kVlen) break;
            for (unsigned i = 0; i < n_new; ++i, ++k) {
                iov[k] = seg ? cut_iov(tr, 0, tr.count) : cut_iov(tr, i, 1);
                set_dst(&dst[k], tr.peer);
                msgs[k] = mmsghdr{};
                msghdr &h = msgs[k].msg_hdr;
                h.msg_name = &dst[k];
                h.msg_namelen = sizeof dst[k];
                h.msg_iov = &iov[k];
                h.msg_iovlen = 1;
                if (seg) {
                    memset(ctl[k].buf, 0, sizeof ctl[k].buf);
                    h.msg_control = ctl[k].buf;
                    h.msg_controllen = sizeof ctl[k].buf;
                    cmsghdr *cm = CMSG_FIRSTHDR(&h);
                    cm->cmsg_level = SOL_UDP;
                    cm->cmsg_type = UDP_SEGMENT;
                    cm->cmsg_len = CMSG_LEN(sizeof(uint16_t));
                    const uint16_t seg_len = (uint16_t)tr.seg_len;
                    memcpy(CMSG_DATA(cm), &seg_len, sizeof seg_len);
                }
                msg_train[k] = next;
                msg_dgrams[k] = seg ? tr.count : 1u;
            }
        }
        for (unsigned done = 0; done < k;) {
            const int r = sendmmsg(fd, msgs.data() + done, k - done, 0);
            if (r >= 0) {
                for (int i = 0; i < r; ++i) {
                    sent += msg_dgrams[done + i];
                    n_seg += msg_dgrams[done + i] > 1;
                }
                n_msgs += (uint64_t)r;
                done += (unsigned)r;
                continue;
            }
            if (errno == EINTR) continue;
            // msgs[done] is the one that failed
            const bool unsupported = errno == ENOPROTOOPT || errno == EOPNOTSUPP;
            const bool refused = unsupported || errno == EINVAL || errno == EIO || errno == EMSGSIZE;
            if (msg_dgrams[done] == 1 || !refused) return finish(true);
            ++n_fell;
            if (!send_singles(ptrains[msg_train[done]])) return finish(true);
            ++done;
            if (unsupported) {
                // this socket takes no UDP_SEGMENT at all: the trains queued behind this one, and the rest
                // of the call, go unsegmented without asking again
                gso = false;
                if (done < k) next = msg_train[done];
                break;
            }
        }
    }
    return finish(false);
}

// socket/udp.go:49-70 plus the UDP_GRO option: the kernel then hands a train of equal-length datagrams of one
// sender back as one buffer (qgcm_udp_recv_gro).
int qgcm_udp_gro(int fd, int on) {
    const int v = on ? 1 : 0;
    return setsockopt(fd, SOL_UDP, UDP_GRO, &v, sizeof v) == 0 ? 0 : -errno;
}

// socket/udp.go:35-41 for coalesced buffers: one recvmsg per buffer, straight into the packed area, one
// table entry each.  The contract is in include/qgcm.h.
int qgcm_udp_recv_gro(int fd, uint8_t *packed, uint64_t packed_cap, qgcm_gro_buf *bufs, uint32_t max_bufs,
                      uint32_t max_n, int timeout_ms, uint64_t out[3]) {
    if (out) out[0] = out[1] = out[2] = 0;
    if (fd < 0 || !packed || !bufs || packed_cap < kGroRoom || max_bufs == 0 || max_n < QGCM_GRO_SEGS) return -1;
    pollfd p{fd, POLLIN, 0};
    int pr;
    do {
        pr = poll(&p, 1, timeout_ms);
    } while (pr < 0 && errno == EINTR);
    if (pr < 0) return -1;
    if (pr == 0) return 0;
    max_n = std::min<uint32_t>(max_n, 0x7fffffffu);       // the count is returned as an int
    packed_cap = std::min<uint64_t>(packed_cap, 1ull << 32);  // offsets are 32-bit
    uint64_t fill = 0, used = 0, cut = 0;
    uint32_t nb = 0, n = 0;
    bool failed = false;
    while (fill + kGroRoom <= packed_cap && nb < max_bufs && max_n - n >= QGCM_GRO_SEGS) {
        alignas(cmsghdr) char ctl[CMSG_SPACE(sizeof(int))];
        iovec iov{packed + fill, (size_t)kGroRoom};
        msghdr h{};
        h.msg_iov = &iov;
        h.msg_iovlen = 1;
        h.msg_control = ctl;
        h.msg_controllen = sizeof ctl;
        const ssize_t r = recvmsg(fd, &h, MSG_DONTWAIT);
        if (r < 0) {
            if (errno == EINTR) continue;
            failed = errno != EAGAIN && errno != EWOULDBLOCK;
            break;
        }
        uint32_t seg = 0;
        for (cmsghdr *cm = CMSG_FIRSTHDR(&h); cm; cm = CMSG_NXTHDR(&h, cm))
            if (cm->cmsg_level == SOL_UDP && cm->cmsg_type == UDP_GRO && cm->cmsg_len >= CMSG_LEN(sizeof(uint16_t))) {
                if (cm->cmsg_len >= CMSG_LEN(sizeof(int))) {
                    int v;
                    memcpy(&v, CMSG_DATA(cm), sizeof v);
                    seg = v > 0 ? (uint32_t)v : 0;
                } else {
                    uint16_t v;
                    memcpy(&v, CMSG_DATA(cm), sizeof v);
                    seg = v;
                }
            }
        uint32_t len = (uint32_t)r;
        uint64_t count = qgcm::gro_count(len, seg);
        if (count > max_n - n) {  // never silent: the datagrams that found no slot are counted
            cut += count - (max_n - n);
            count = max_n - n;
            len = (uint32_t)count * seg;
        }
        bufs[nb++] = qgcm_gro_buf{(uint32_t)fill, len, seg, n};
        n += (uint32_t)count;
        used = fill + len;
        fill = (used + 15) & ~(uint64_t)15;
    }
    if (out) {
        out[0] = nb;
        out[1] = used;
        out[2] = cut;
    }
    return failed && nb == 0 ? -1 : (int)n;
}

// The delivered packets of an opened batch packed back to back by the host (pack_core.h; the contract of
// qgcm_deliver_pack, no alignment asked): what a worker on qgcm_route_chain_open_host hands to
// qgcm_tun_write_packed.
int qgcm_deliver_pack_cpu(const uint8_t *arena, uint64_t stride, uint32_t n, const uint32_t *lens, const uint32_t *peer,
                          const uint8_t *status, uint8_t *packed, uint64_t packed_cap, qgcm_pack_rec *recs,
                          uint64_t counts[2]) {
    if (n > QGCM_MAX_BATCH || (stride & 3) || packed_cap > qgcm::kPackMaxCap || !counts) return QGCM_E_ARG;
    if (n && (!arena || !lens || !peer || !packed || !recs || stride == 0)) return QGCM_E_ARG;
    qgcm::deliver_pack_cpu(arena, stride, n, lens, peer, status, packed, packed_cap, recs, counts);
    return QGCM_OK;
}

// The delivered TCP segments of an opened batch coalesced by the host (coalesce_core.h; the contract of
// qgcm_deliver_coalesce, no alignment asked): what a worker on qgcm_route_chain_open_host hands to
// qgcm_tun_write_gso.
int qgcm_deliver_coalesce_cpu(const uint8_t *arena, uint64_t stride, uint32_t n, const uint32_t *lens, const uint32_t *peer,
                              const uint8_t *status, uint8_t *packed, uint64_t packed_cap, qgcm_gso_frame *frames,
                              uint64_t counts[4]) {
    if (n > QGCM_MAX_BATCH || (stride & 3) || packed_cap > qgcm::kPackMaxCap || !counts) return QGCM_E_ARG;
    if (n && (!arena || !lens || !peer || !packed || !frames || stride == 0)) return QGCM_E_ARG;
    std::vector<uint32_t> work;
    try {
        work.resize(2 * (size_t)n);
    } catch (...) {
        return QGCM_E_NOMEM;
    }
    qgcm::deliver_coalesce_cpu(arena, stride, n, lens, peer, status, packed, packed_cap, frames, counts, work.data(),
                               work.data() + n);
    return QGCM_OK;
}

// The trains of a planned batch packed back to back by the host (train_core.h; the contract of qgcm_train_pack,
// no alignment asked, the plan checked whole first): what a worker on qgcm_route_chain_seal_host hands to
// qgcm_udp_send_packed.
int qgcm_train_pack_cpu(const uint8_t *arena, uint64_t stride, uint32_t n, const uint32_t *order, uint32_t m,
                        const qgcm_train *trains, uint32_t t, uint8_t *packed, uint64_t packed_cap,
                        qgcm_ptrain *ptrains, uint64_t pcounts[2]) {
    if (n > QGCM_MAX_BATCH || (stride & 3) || packed_cap > qgcm::kTrainMaxCap || !pcounts) return QGCM_E_ARG;
    if (n && (!arena || !order || !trains || !packed || !ptrains || stride == 0)) return QGCM_E_ARG;
    if ((m && !order) || (t && (!trains || !ptrains || !arena || !packed))) return QGCM_E_ARG;
    if (!qgcm::train_plan_ok(stride, n, order, m, trains, t)) return QGCM_E_ARG;
    qgcm::train_pack_cpu(arena, stride, order, trains, t, packed, packed_cap, ptrains, pcounts);
    return QGCM_OK;
}

// Split DTLS records (include/qgcm.h "DTLS 1.2 records on routed batches"), one record per datagram: the 21
// bytes of hdr[i] in front of Raw[:lens[i]] of slot i by a second iovec, so neither side copies a record
// together.  To addrs[peer[i]] for the slots with status 1, as qgcm_udp_send_slots_to.
int qgcm_udp_send_dtls(int fd, const uint8_t *arena, uint64_t stride, uint32_t n, const uint32_t *lens,
                       const qgcm_dtls_hdr *hdr, const uint8_t *status, const uint32_t *peer,
                       const qgcm_peer_addr *addrs, uint32_t n_addrs) {
    if (fd < 0 || (n && (!arena || !lens || !hdr || !peer)) || (n_addrs && !addrs)) return -1;
    auto skip = [&](uint32_t i) { return (status && status[i] != 1) || peer[i] == QGCM_NO_PEER || lens[i] == 0; };
    for (uint32_t i = 0; i < n; ++i)
        if (!skip(i) && peer[i] >= n_addrs) return -1;
    std::vector<mmsghdr> msgs(kVlen);
    std::vector<iovec> iov(2 * kVlen);
    std::vector<sockaddr_in> dst(kVlen);
    uint32_t next = 0, sent = 0;
    while (next < n) {
        unsigned k = 0;
        for (; next < n && k < kVlen; ++next) {
            if (skip(next)) continue;
            const qgcm_peer_addr &a = addrs[peer[next]];
            memset(&dst[k], 0, sizeof dst[k]);
            dst[k].sin_family = AF_INET;
            dst[k].sin_addr.s_addr = a.ip;  // network byte order already
            dst[k].sin_port = a.port;
            iov[2 * k] = iovec{const_cast<uint8_t *>(hdr[next].b), (size_t)QGCM_DTLS_HDR_BYTES};
            iov[2 * k + 1] = iovec{const_cast<uint8_t *>(arena) + (uint64_t)next * stride,
                                   (size_t)std::min<uint64_t>(lens[next], stride)};
            msgs[k] = mmsghdr{};
            msgs[k].msg_hdr.msg_name = &dst[k];
            msgs[k].msg_hdr.msg_namelen = sizeof dst[k];
            msgs[k].msg_hdr.msg_iov = &iov[2 * k];
            msgs[k].msg_hdr.msg_iovlen = 2;
            ++k;
        }
        for (unsigned done = 0; done < k;) {
            const int r = sendmmsg(fd, msgs.data() + done, k - done, 0);
            if (r < 0) {
                if (errno == EINTR) continue;
                return sent ? (int)sent : -1;
            }
            done += (unsigned)r;
            sent += (uint32_t)r;
        }
    }
    return (int)sent;
}

// The receiving side: datagram -> hdr[i].b[0:21] and Raw[0:lens[i]] of slot i, the sender to addrs_out[i].  A
// datagram that cannot be a record in a slot (under 22 bytes, or longer than 21 + stride: the kernel marks it
// truncated) is dropped and counted; the slots filled stay dense.
int qgcm_udp_recv_dtls(int fd, uint8_t *arena, uint64_t stride, uint32_t max_n, uint32_t *lens, qgcm_dtls_hdr *hdr,
                       qgcm_peer_addr *addrs_out, int timeout_ms, uint32_t *dropped) {
    if (dropped) *dropped = 0;
    if (fd < 0 || (max_n && (!arena || !lens || !hdr)) || stride == 0) return -1;
    if (max_n == 0) return 0;
    pollfd p{fd, POLLIN, 0};
    int pr;
    do {
        pr = poll(&p, 1, timeout_ms);
    } while (pr < 0 && errno == EINTR);
    if (pr < 0) return -1;
    if (pr == 0) return 0;
    const size_t vlen = std::min<uint32_t>(max_n, kVlen);
    std::vector<mmsghdr> msgs(vlen);
    std::vector<iovec> iov(2 * vlen);
    std::vector<sockaddr_in> src(vlen);
    uint32_t got = 0, lost = 0;
    while (got < max_n) {
        const unsigned k = (unsigned)std::min<uint64_t>(max_n - got, vlen);
        for (unsigned i = 0; i < k; ++i) {
            iov[2 * i] = iovec{hdr[got + i].b, (size_t)QGCM_DTLS_HDR_BYTES};
            iov[2 * i + 1] = iovec{arena + (uint64_t)(got + i) * stride, (size_t)stride};
            msgs[i] = mmsghdr{};
            msgs[i].msg_hdr.msg_name = &src[i];
            msgs[i].msg_hdr.msg_namelen = sizeof src[i];
            msgs[i].msg_hdr.msg_iov = &iov[2 * i];
            msgs[i].msg_hdr.msg_iovlen = 2;
        }
        const int r = recvmmsg(fd, msgs.data(), k, MSG_DONTWAIT, nullptr);
        if (r < 0) {
            if (errno == EINTR) continue;
            if (errno == EAGAIN || errno == EWOULDBLOCK) break;
            if (dropped) *dropped = lost;
            return got ? (int)got : -1;
        }
        uint32_t kept = 0;  // of this round: message i moves down to slot got + kept
        for (int i = 0; i < r; ++i) {
            const uint32_t len = msgs[i].msg_len;
            if (len <= QGCM_DTLS_HDR_BYTES || (msgs[i].msg_hdr.msg_flags & MSG_TRUNC)) {
                ++lost;
                continue;
            }
            const uint32_t to = got + kept, from = got + (uint32_t)i, body = len - QGCM_DTLS_HDR_BYTES;
            if (to != from) {
                memcpy(hdr[to].b, hdr[from].b, QGCM_DTLS_HDR_BYTES);
                memcpy(arena + (uint64_t)to * stride, arena + (uint64_t)from * stride, body);
            }
            memset(hdr[to].b + QGCM_DTLS_HDR_BYTES, 0, sizeof hdr[to].b - QGCM_DTLS_HDR_BYTES);
            lens[to] = body;
            if (addrs_out) addrs_out[to] = qgcm_peer_addr{src[i].sin_addr.s_addr, src[i].sin_port, 0};
            ++kept;
        }
        got += kept;
        if ((unsigned)r < k) break;
    }
    if (dropped) *dropped = lost;
    return (int)got;
}

}  // extern "C"
