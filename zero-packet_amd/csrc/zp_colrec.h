// zp_colrec.h — the record decode of the one-lane-per-frame column kernels:
// the 8-B zp_record unpacked into zp_rec_full (both forms, inline chains),
// the header bytes to stage for it, and the fields the record does not carry
// (final_next_header, the far-L4 form's eth_len / inner_off) read from the
// staged frame. Shared by every kernel that reads columns through the window:
// zp_columns_kernel (zp_fields.hip), zp_select_mark_terms_kernel
// (zp_select.hip), zp_classify_kernel (zp_classify.hip), zp_route_kernel
// (zp_route.hip) and both instances of zp_flow_key_kernel (zp_flow.hip). Each
// asks fx_rec_need() for its own column groups, so the same frame's window
// ends elsewhere in each of them (tests/test_window_stages.py).
#pragma once
#include "zp_cols.h"
#include "zp_win.h"

// IPv6Reader::final_next_header (ipv6.rs:219-227) of the IPv6 header at
// `ip`: its next-header byte, or with an extension chain the next-header
// byte of the chain's last header (headers.rs:51-213 stops after the
// headers the slot bits name; lengths by type as in the walk).
// *end = the upper-layer payload's start (ipv6.rs:283-285).
template <class R>
__device__ __forceinline__ uint32_t final_nh(R& rd, uint32_t ip, uint32_t slots, uint32_t* end) {
    uint32_t cur = rd(ip + 6), p = ip + 40;
    for (int k = __builtin_popcount(slots & 63u); k > 0; --k) {
        const uint32_t b1 = rd(p + 1);
        const uint32_t hl = cur == 44 ? 8u : cur == 51 ? (b1 + 2) * 4 : (b1 + 1) * 8;
        cur = rd(p);
        p += hl;
    }
    *end = p;
    return cur;
}

// The 8-B record q, unpacked (include/zero_packet.h); the final next headers
// of the IPv6 readers come from the frame after the staging (fx_rec_finish).
// Returns whether the record has the far-L4 form (an L4 reader past byte
// 262,143): offs holds the whole L4 offset; the Ethernet header length and
// inner_off are read from the frame after the staging.
__device__ __forceinline__ bool fx_rec_decode(const zp_u32x2& q, zp_rec_full& r) {
    r.flags = q.x & ZP_F_MASK;
    r.err = (uint8_t)(q.x >> 26);
    r.final_nh = 0;
    r.inner_final_nh = 0;
    const bool far = ((q.x >> 24) & 3u) == ZP_ETH_CODE_FAR;
    r.eth_len = (uint8_t)(far ? 22u : 14u + 4u * ((q.x >> 24) & 3u));
    r.l4_off = far ? q.y : q.y & ZP_L4_NEAR_MAX;
    r.inner_off = far || !(r.flags & ZP_F_IP_IN_IP) ? 0u : q.y >> 18;   // else: an inline chain
    r.chain = 0;
    return far;
}

// The header bytes the getters read: the last header the record names ends by
// l4 + 20 (TCP) / inner + 40 / l3 + 40. l3 / inner / l4: whether that group's
// getters run at all (ColStore: all three).
__device__ __forceinline__ uint32_t fx_rec_need(const zp_rec_full& r, bool ok, bool far, bool l3,
                                                bool inner, bool l4) {
    uint32_t need = 22;
    if (ok) {
        const uint32_t e3 = r.eth_len + 40;
        if (l3) need = e3 > need ? e3 : need;
        if (inner && (r.flags & ZP_F_IP_IN_IP))
            need = r.inner_off + 40 > need ? r.inner_off + 40 : need;
        if (l4 && (r.flags & (ZP_F_TCP | ZP_F_UDP | ZP_F_ICMPV4 | ZP_F_ICMPV6)))
            need = r.l4_off + 20 > need ? r.l4_off + 20 : need;
    }
    if (far) need = FX_WIN;             // eth_len / inner_off not known yet
    return need;
}

// After the staging: the far-L4 form's Ethernet header length and inner_off,
// and the final next headers of the IPv6 readers.
template <class R>
__device__ __forceinline__ void fx_rec_finish(R& rd, zp_rec_full& r, bool ok, bool far) {
    if (ok && far) {
        const uint32_t t0 = rd16(rd, 12u);                          // ethernet.rs:155-179
        r.eth_len = (uint8_t)(t0 == 0x8100 ? 18u : t0 == 0x88A8 ? 22u : 14u);
    }
    uint32_t ulp = 0;
    if (ok && (r.flags & ZP_F_IPV6))
        r.final_nh = (uint8_t)final_nh(rd, r.eth_len, r.flags >> 12, &ulp);
    if (ok && far)                      // ip_in_ip follows the outer IP header
        r.inner_off = (r.flags & ZP_F_IPV6) ? ulp : r.eth_len + (rd(r.eth_len) & 15u) * 4u;
    if (ok && (r.flags & ZP_F_IP_IN_IP_V6))
        r.inner_final_nh = (uint8_t)final_nh(rd, r.inner_off, r.flags >> 18, &ulp);
}
