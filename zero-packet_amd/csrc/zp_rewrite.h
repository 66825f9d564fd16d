// zp_rewrite.h — the writers' field setters over one parsed frame
// (include/zero_packet.h, zp_rewrite_columns_device): entry i of every given
// column is written into the frame where the extract of that column would
// read a present reader, and the IPv4 header checksum and the L4 checksum are
// updated from the changed 16-bit words alone (RFC 1624; an L4 slice of
// ZP_REWRITE_EXACT_L4_BYTES or more is summed in full instead). `rd(x)`
// returns the frame's old byte x from wherever the caller staged it; `g` is the frame in
// global memory (a pointer to uint8_t, in the global address space if the
// caller knows it). Frames sit at any alignment and share dwords with their
// neighbours, so every store covers exactly the bytes of its field: byte
// stores, which the compiler may merge into one unaligned store of bytes that
// are all written anyway, never a read-modify-write of a wider unit.
#pragma once
#include "zp_cols.h"

template <typename T>
__device__ __forceinline__ T ldc(const ColPtrs& c, int col, uint64_t i) {
    return ((const T*)c.p[col])[i];
}

template <class P>
__device__ __forceinline__ void st_be16(P g, uint32_t x, uint32_t v) {
    g[x] = (uint8_t)(v >> 8);
    g[x + 1] = (uint8_t)v;
}
template <class P>
__device__ __forceinline__ void st_be32(P g, uint32_t x, uint32_t v) {
    g[x] = (uint8_t)(v >> 24);
    g[x + 1] = (uint8_t)(v >> 16);
    g[x + 2] = (uint8_t)(v >> 8);
    g[x + 3] = (uint8_t)v;
}

// The running update of one checksum: acc = sum of (~m + m') over the covered
// big-endian words written so far, chg = some word got another value.
struct RwSum {
    uint32_t acc;
    bool chg;
};
__device__ __forceinline__ void rw_word(RwSum& s, uint32_t o, uint32_t n) {
    s.acc += (~o & 0xFFFFu) + n;
    s.chg |= o != n;
}
__device__ __forceinline__ void rw_add(RwSum& s, const RwSum& d) {
    s.acc += d.acc;
    s.chg |= d.chg;
}
// The new checksum from the stored one: T = ~C + acc folded with end-around
// carry, 0 counted as 0xFFFF, complemented. For a frame that verified this is
// the writers' full recompute (T = S' mod 65535, both in
// [1, 0xFFFF]) as long as the reference's u32 sum cannot wrap: every IPv4
// header, and an L4 slice below ZP_REWRITE_EXACT_L4_BYTES. acc holds at most
// 40 words, so two folds suffice.
__device__ __forceinline__ uint32_t rw_checksum(uint32_t c, const RwSum& s) {
    uint32_t t = (~c & 0xFFFFu) + s.acc;
    t = (t & 0xFFFFu) + (t >> 16);
    t = (t & 0xFFFFu) + (t >> 16);
    if (t == 0) t = 0xFFFFu;
    return ~t & 0xFFFFu;
}

// The L4 checksum of a long slice (len - p >= ZP_REWRITE_EXACT_L4_BYTES), the
// way the L4 writers' set_checksum(pseudo_sum) computes it (tcp.rs:123-129,
// icmpv4.rs:74-80, icmpv6.rs:71-77): the full word sum of the NEW slice
// g[p, len) with the checksum field at ck counted as zero, plus the
// pseudo-header of the innermost IP header, in the reference's wrapping u32
// (checksum.rs:5-29). A sum that may reach 2^32 is not a sum mod 65535 (every
// wrap shifts the folded value by one, and a wrapped sum of 0 folds to 0), so
// rw_checksum does not serve these frames. Called after the frame's field
// stores, by the lane that made them; the lane alone reads its slice, in
// aligned 16-B chunks (the bytes outside [p, len) masked out), summing the
// bytes at even and odd addresses apart as the parse's exact path does.
// Only an IPv6 header can sit in front of such a slice (parser.rs:203 bounds
// an IPv4 payload by its 16-bit total length), its protocol is the L4
// reader's (parser.rs:96-98), and UDP does not occur (parser.rs:261).
template <class P>
__device__ __forceinline__ uint32_t rw_l4_exact(P g, uint32_t flags, uint32_t hl, uint32_t p,
                                                uint32_t len, uint32_t ck, uint32_t l4f,
                                                uint32_t fallback) {
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    // the innermost IP header: the one whose payload starts at p. An accepted
    // frame's chain has no errors, so the walk only needs the header lengths
    // (ipv4.rs IHL; headers.rs:51-213: the five extension types, each once,
    // Destination Options twice).
    uint32_t pos = hl;
    if (flags & ZP_F_IP_IN_IP) {
        bool found = false;
        while (!found && pos + 40u <= p) {
            uint32_t nxt, proto;
            if ((g[pos] >> 4) == 4) {
                nxt = pos + (g[pos] & 15u) * 4u;
                proto = g[pos + 9];
            } else {
                uint32_t pres = 0;
                nxt = pos + 40u;
                proto = g[pos + 6];
                for (int it = 0; it < 7; ++it) {
                    const uint32_t bit = proto == 0 ? 1u : proto == 43 ? 2u : proto == 44 ? 4u
                                       : proto == 51 ? 8u
                                       : proto == 60 ? ((pres & 16u) ? 32u : 16u) : 0u;
                    if (bit == 0 || (pres & bit) || nxt + 8u > p) break;
                    const uint32_t b1 = g[nxt + 1];
                    pres |= bit;
                    proto = g[nxt];
                    nxt += bit == 4u ? 8u : bit == 8u ? (b1 + 2u) * 4u : (b1 + 1u) * 8u;
                }
            }
            if (nxt == p && proto != 4 && proto != 41) found = true;
            else if (nxt <= pos || nxt > p || (proto != 4 && proto != 41)) break;
            else pos = nxt;
        }
        if (!found) return fallback;         // not reached for a frame the parse accepted
    }
    if ((g[pos] >> 4) != 6 || pos + 40u > p) return fallback;     // as above
    uint32_t acc = (l4f == ZP_F_TCP ? 6u : l4f == ZP_F_ICMPV4 ? 1u : 58u) + (len - p);   // checksum.rs:67-69
    for (uint32_t k = 0; k < 32; k += 2) acc += ((uint32_t)g[pos + 8 + k] << 8) | g[pos + 9 + k];
    const uintptr_t a0 = (uintptr_t)g + p, a1 = (uintptr_t)g + len;
    uint64_t E = 0, O = 0;                   // byte sums at even / odd addresses
    for (uintptr_t d = a0 & ~(uintptr_t)15; d < a1; d += 16) {
        const u32x4 q = *(const __attribute__((address_space(1))) u32x4*)d;
        uint32_t v[4] = {q.x, q.y, q.z, q.w};
        if (d < a0 || a1 - d < 16) {         // the slice's first and last chunk
            const uint32_t lo = d < a0 ? (uint32_t)(a0 - d) : 0u;
            const uint32_t hi = a1 - d < 16 ? (uint32_t)(a1 - d) : 16u;
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) {
                uint32_t m = 0;
#pragma unroll
                for (uint32_t b = 0; b < 4; ++b)
                    if (4 * k + b >= lo && 4 * k + b < hi) m |= 0xFFu << (8 * b);
                v[k] &= m;
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            E += (v[k] & 0xFFu) + ((v[k] >> 16) & 0xFFu);
            O += ((v[k] >> 8) & 0xFFu) + (v[k] >> 24);
        }
    }
    // words start at p; the checksum field (even from p) counts as zero
    const uint64_t W = ((a0 & 1) ? 256ull * O + E : 256ull * E + O) -
                       (((uint32_t)g[ck] << 8) | g[ck + 1]);
    uint32_t S = (uint32_t)(acc + W);                                  // checksum.rs:12: u32 wrap
    while (S >> 16) S = (S & 0xFFFFu) + (S >> 16);
    return ~S & 0xFFFFu;
}

// One big-endian 16-bit / 32-bit field at x (even from its header's start).
template <class R, class P>
__device__ __forceinline__ void put16(R& rd, P g, uint32_t x, uint32_t v, RwSum& s) {
    rw_word(s, rd16(rd, x), v);
    st_be16(g, x, v);
}
template <class R, class P>
__device__ __forceinline__ void put32(R& rd, P g, uint32_t x, uint32_t v, RwSum& s) {
    const uint32_t o = rd32(rd, x);
    rw_word(s, o >> 16, v >> 16);
    rw_word(s, o & 0xFFFFu, v & 0xFFFFu);
    st_be32(g, x, v);
}
// Bytes [x, x + 4 * nw) from nw + nw2 dwords in frame byte order (an address
// entry, or the source and destination entries of adjacent address fields):
// all old words are read first, so the byte stores follow each other and the
// compiler merges them into stores of up to 16 B. d = their update.
template <class R, class P>
__device__ __forceinline__ void put_addr(R& rd, P g, uint32_t x, const uint4& a, int nw,
                                         const uint4& b, int nw2, RwSum& d) {
    const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    uint32_t v[8];
    int m = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if ((k < 4 && k < nw) || (k >= 4 && k - 4 < nw2)) v[m++] = w[k];
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if (k < m) {
            const uint32_t o = rd32(rd, x + 4 * k), n = __builtin_bswap32(v[k]);
            rw_word(d, o >> 16, n >> 16);
            rw_word(d, o & 0xFFFFu, n & 0xFFFFu);
        }
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if (k < m) {
            g[x + 4 * k] = (uint8_t)v[k];
            g[x + 4 * k + 1] = (uint8_t)(v[k] >> 8);
            g[x + 4 * k + 2] = (uint8_t)(v[k] >> 16);
            g[x + 4 * k + 3] = (uint8_t)(v[k] >> 24);
        }
}

// Frame of record (flags, Ethernet header length hl, L4 offset p), accepted
// by the parse with an Ethernet reader; len = its length.
template <class R, class P>
__device__ __forceinline__ void rewrite_frame(R& rd, P g, uint32_t flags, uint32_t hl,
                                              uint32_t p, uint32_t len, uint64_t i,
                                              const ColPtrs& c) {
    // Adjacent fields that are both written go out in one run of byte stores
    // (one store instruction after merging): the two MACs, the two addresses,
    // the TCP ports with the sequence and acknowledgment numbers.
    if (c.p[ZP_COL_DEST_MAC] || c.p[ZP_COL_SRC_MAC]) {                // ethernet.rs:47, :58
        uint32_t v[6] = {0u, 0u, 0u, 0u, 0u, 0u};
        if (c.p[ZP_COL_DEST_MAC]) {
            const uint16_t* s = (const uint16_t*)(c.p[ZP_COL_DEST_MAC] + 6 * i);
            v[0] = s[0]; v[1] = s[1]; v[2] = s[2];
        }
        if (c.p[ZP_COL_SRC_MAC]) {
            const uint16_t* s = (const uint16_t*)(c.p[ZP_COL_SRC_MAC] + 6 * i);
            v[3] = s[0]; v[4] = s[1]; v[5] = s[2];
        }
        if (c.p[ZP_COL_DEST_MAC] && c.p[ZP_COL_SRC_MAC]) {
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                g[2 * k] = (uint8_t)v[k];
                g[2 * k + 1] = (uint8_t)(v[k] >> 8);
            }
        } else if (c.p[ZP_COL_DEST_MAC]) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                g[2 * k] = (uint8_t)v[k];
                g[2 * k + 1] = (uint8_t)(v[k] >> 8);
            }
        } else {
#pragma unroll
            for (int k = 3; k < 6; ++k) {
                g[2 * k] = (uint8_t)v[k];
                g[2 * k + 1] = (uint8_t)(v[k] >> 8);
            }
        }
    }
    if (c.p[ZP_COL_VLAN_TCI] || c.p[ZP_COL_VLAN_INNER_TCI]) {         // ethernet.rs:83-129
        const uint32_t tp = rd16(rd, 12);
        if (c.p[ZP_COL_VLAN_TCI]) {
            const uint32_t v = ldc<uint16_t>(c, ZP_COL_VLAN_TCI, i);
            if ((tp == 0x8100 || tp == 0x88A8) && hl >= 18) st_be16(g, 14, v);
        }
        if (c.p[ZP_COL_VLAN_INNER_TCI]) {
            const uint32_t v = ldc<uint16_t>(c, ZP_COL_VLAN_INNER_TCI, i);
            if (tp == 0x88A8 && hl >= 22) st_be16(g, 18, v);
        }
    }

    const uint32_t l4f = flags & (ZP_F_TCP | ZP_F_UDP | ZP_F_ICMPV4 | ZP_F_ICMPV6);
    const bool v6 = (flags & ZP_F_IPV6) != 0;
    const bool ip = (flags & (ZP_F_IPV4 | ZP_F_IPV6)) && len >= hl + (v6 ? 40u : 20u);
    RwSum s3 = {0u, false}, s4 = {0u, false};    // IPv4 header checksum, L4 checksum
    // The L4 checksum covers the outer addresses when the outer reader is the
    // one that verified it (parser.rs:311-362): no ip_in_ip, and not ICMPv4
    // under IPv4 (acc = 0).
    const bool pseudo = l4f && !(flags & ZP_F_IP_IN_IP) && (v6 || l4f != ZP_F_ICMPV4);
    uint4 sa = make_uint4(0, 0, 0, 0), da = sa;
    uint32_t ttl = 0, tos = 0, id = 0;
    if (c.p[ZP_COL_SRC_ADDR]) sa = ldc<uint4>(c, ZP_COL_SRC_ADDR, i);
    if (c.p[ZP_COL_DEST_ADDR]) da = ldc<uint4>(c, ZP_COL_DEST_ADDR, i);
    if (c.p[ZP_COL_TTL]) ttl = ldc<uint8_t>(c, ZP_COL_TTL, i);
    if (c.p[ZP_COL_TOS]) tos = ldc<uint8_t>(c, ZP_COL_TOS, i);
    if (c.p[ZP_COL_IP_ID]) id = ldc<uint32_t>(c, ZP_COL_IP_ID, i);
    if (ip && !v6) {
        if (c.p[ZP_COL_TOS]) {                                        // ipv4.rs:46-54
            const uint32_t o = rd16(rd, hl);
            rw_word(s3, o, (o & 0xFF00u) | tos);
            g[hl + 1] = (uint8_t)tos;
        }
        if (c.p[ZP_COL_IP_ID]) put16(rd, g, hl + 4, id & 0xFFFFu, s3);   // ipv4.rs:67
        if (c.p[ZP_COL_TTL]) {                                        // ipv4.rs:87
            const uint32_t o = rd16(rd, hl + 8);
            rw_word(s3, o, (o & 0xFFu) | (ttl << 8));
            g[hl + 8] = (uint8_t)ttl;
        }
        RwSum d = {0u, false};
        if (c.p[ZP_COL_SRC_ADDR] && c.p[ZP_COL_DEST_ADDR])             // ipv4.rs:99-113
            put_addr(rd, g, hl + 12, sa, 1, da, 1, d);
        else if (c.p[ZP_COL_SRC_ADDR]) put_addr(rd, g, hl + 12, sa, 1, sa, 0, d);
        else if (c.p[ZP_COL_DEST_ADDR]) put_addr(rd, g, hl + 16, da, 1, da, 0, d);
        rw_add(s3, d);
        if (pseudo) rw_add(s4, d);
        if (s3.chg)                                                   // ipv4.rs:119-126
            st_be16(g, hl + 10, rw_checksum(rd16(rd, hl + 10), s3));
    } else if (ip) {
        if (c.p[ZP_COL_TOS] || c.p[ZP_COL_IP_ID]) {
            uint32_t b1 = rd(hl + 1);
            if (c.p[ZP_COL_TOS]) {                                    // ipv6.rs:42
                g[hl] = (uint8_t)((rd(hl) & 0xF0u) | (tos >> 4));
                b1 = (b1 & 0x0Fu) | ((tos << 4) & 0xF0u);
            }
            if (c.p[ZP_COL_IP_ID]) {                                  // ipv6.rs:51
                b1 = (b1 & 0xF0u) | ((id >> 16) & 0x0Fu);
                st_be16(g, hl + 2, id & 0xFFFFu);
            }
            g[hl + 1] = (uint8_t)b1;
        }
        if (c.p[ZP_COL_TTL]) g[hl + 7] = (uint8_t)ttl;                // ipv6.rs:84
        RwSum d = {0u, false};
        if (c.p[ZP_COL_SRC_ADDR] && c.p[ZP_COL_DEST_ADDR])             // ipv6.rs:92-133
            put_addr(rd, g, hl + 8, sa, 4, da, 4, d);
        else if (c.p[ZP_COL_SRC_ADDR]) put_addr(rd, g, hl + 8, sa, 4, sa, 0, d);
        else if (c.p[ZP_COL_DEST_ADDR]) put_addr(rd, g, hl + 24, da, 4, da, 0, d);
        if (pseudo) rw_add(s4, d);
    }

    const bool tcp = l4f == ZP_F_TCP, udp = l4f == ZP_F_UDP;
    uint32_t sp = 0, dp = 0, seq = 0, ack = 0, wnd = 0;
    if (c.p[ZP_COL_SRC_PORT]) sp = ldc<uint16_t>(c, ZP_COL_SRC_PORT, i);
    if (c.p[ZP_COL_DEST_PORT]) dp = ldc<uint16_t>(c, ZP_COL_DEST_PORT, i);
    if (c.p[ZP_COL_TCP_SEQ]) seq = ldc<uint32_t>(c, ZP_COL_TCP_SEQ, i);
    if (c.p[ZP_COL_TCP_ACK]) ack = ldc<uint32_t>(c, ZP_COL_TCP_ACK, i);
    if (c.p[ZP_COL_TCP_WINDOW]) wnd = ldc<uint16_t>(c, ZP_COL_TCP_WINDOW, i);
    const uint32_t hmin = tcp ? 20u : udp ? 8u : 4u;
    if (l4f && len >= hmin && p <= len - hmin) {
        const bool ports = c.p[ZP_COL_SRC_PORT] && c.p[ZP_COL_DEST_PORT];
        const bool nums = c.p[ZP_COL_TCP_SEQ] && c.p[ZP_COL_TCP_ACK];
        if (tcp && ports && nums) {             // tcp.rs:37-60: bytes [p, p + 12) in one run
            const uint32_t n0 = (sp << 16) | dp;
            const uint32_t o0 = rd32(rd, p), o1 = rd32(rd, p + 4), o2 = rd32(rd, p + 8);
            rw_word(s4, o0 >> 16, sp);
            rw_word(s4, o0 & 0xFFFFu, dp);
            rw_word(s4, o1 >> 16, seq >> 16);
            rw_word(s4, o1 & 0xFFFFu, seq & 0xFFFFu);
            rw_word(s4, o2 >> 16, ack >> 16);
            rw_word(s4, o2 & 0xFFFFu, ack & 0xFFFFu);
            st_be32(g, p, n0);
            st_be32(g, p + 4, seq);
            st_be32(g, p + 8, ack);
        } else {
            if ((tcp || udp) && ports) {                              // tcp.rs:37-50, udp.rs:37-50
                put32(rd, g, p, (sp << 16) | dp, s4);
            } else if (tcp || udp) {
                if (c.p[ZP_COL_SRC_PORT]) put16(rd, g, p, sp, s4);
                if (c.p[ZP_COL_DEST_PORT]) put16(rd, g, p + 2, dp, s4);
            }
            if (tcp) {
                if (c.p[ZP_COL_TCP_SEQ]) put32(rd, g, p + 4, seq, s4);   // tcp.rs:51
                if (c.p[ZP_COL_TCP_ACK]) put32(rd, g, p + 8, ack, s4);   // tcp.rs:60
            }
        }
        if (tcp && c.p[ZP_COL_TCP_WINDOW]) put16(rd, g, p + 14, wnd, s4);    // tcp.rs:87
        // tcp.rs:123-129, udp.rs:65-71, icmpv4.rs:74-80, icmpv6.rs:71-77
        const uint32_t ck = p + (tcp ? 16u : udp ? 6u : 2u);
        if (s4.chg) {
            uint32_t v = rw_checksum(rd16(rd, ck), s4);
            // a slice long enough for the reference's u32 sum to wrap: the
            // full recompute (rare: IPv6 jumbograms only)
            if (__builtin_expect(len - p >= ZP_REWRITE_EXACT_L4_BYTES, 0))
                v = rw_l4_exact(g, flags, hl, p, len, ck, l4f, v);
            st_be16(g, ck, v);
        }
    }
}
