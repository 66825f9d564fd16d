// zp_fields.hip — column views over parsed frames.
//
// zp_extract_columns_device gathers the reader getters of every parsed frame
// (EthernetReader ethernet.rs:195-244, ArpReader::oper arp.rs:174-177,
// IPv4Reader ipv4.rs:148-219, IPv6Reader ipv6.rs:173-256, TcpReader
// tcp.rs:151-243, UdpReader udp.rs:113-154, Icmpv4/6Reader icmpv4.rs:102-135,
// icmpv6.rs:99-132) into SoA device columns, driven by the zp_record the
// parse kernel wrote: offsets say where each reader starts, flags which
// readers exist. Column semantics: include/zero_packet.h (zp_col).
//
// One lane per frame, 256 frames per workgroup. Each lane stages the first
// 128 B of its frame (from A & ~15) in LDS with 16-B loads; headers past the
// window (deep IPv6 chains, IP-in-IP) are read from global memory. Column
// stores are one element per lane, coalesced across the wave. HBM-bound:
// per frame one or two 128-B lines in, sum of the requested column widths out.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/zero_packet.h"
#include "zp_cols.h"
#include "zp_win.h"                      // FX_WIN, the staged window and its reader

extern "C" char* zp__errbuf(void);

static const int kColWidth[ZP_COL_COUNT] = {
    6, 6, 2, 2, 2, 2, 1, 16, 16, 1, 1, 1, 4, 2, 1, 16, 16, 1, 1, 2, 2, 4, 4, 1, 2, 1, 1, 2, 4};

extern "C" int zp_col_width(int col) {
    return col >= 0 && col < ZP_COL_COUNT ? kColWidth[col] : 0;
}

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

__global__ void __launch_bounds__(FX_BLOCK)
zp_columns_kernel(const uint8_t* __restrict__ arena, const uint64_t* __restrict__ offs,
                  const uint32_t* __restrict__ lens, const zp_record* __restrict__ recs,
                  uint64_t n, ColPtrs c) {
    __shared__ uint4 win[FX_CH * FX_BLOCK];
    const uint64_t i0 = (uint64_t)blockIdx.x * FX_BLOCK + threadIdx.x;
    // Lanes past the batch stay for the cooperative staging (no wave exits
    // early: ds_bpermute reads every lane); they load and store nothing.
    const bool live = i0 < n;
    const uint64_t i = live ? i0 : n - 1;
    // the 8-B record, unpacked (include/zero_packet.h); the final next
    // headers of the IPv6 readers come from the frame after the staging
    zp_rec_full r;
    static_assert(sizeof(zp_record) == 8, "one 8-B load per record");
    const zp_u32x2 q = *(const FX_GLOBAL zp_u32x2*)(recs + i);
    r.flags = q.x & ZP_F_MASK;
    r.err = (uint8_t)(q.x >> 26);
    r.final_nh = 0;
    r.inner_final_nh = 0;
    // The far-L4 form (an L4 reader past byte 262,143): offs holds the whole
    // L4 offset; the Ethernet header length and inner_off are read from the
    // frame after the staging (include/zero_packet.h).
    const bool far = ((q.x >> 24) & 3u) == ZP_ETH_CODE_FAR;
    r.eth_len = (uint8_t)(far ? 22u : 14u + 4u * ((q.x >> 24) & 3u));
    r.l4_off = far ? q.y : q.y & ZP_L4_NEAR_MAX;
    r.inner_off = far || !(r.flags & ZP_F_IP_IN_IP) ? 0u : q.y >> 18;   // else: an inline chain
    r.chain = 0;
    const bool ok = live && r.err == 0 && (r.flags & ZP_F_ETHERNET);
    const uint32_t len = ok ? lens[i] : 0u;
    const uintptr_t ga = (uintptr_t)arena + (ok ? offs[i] : 0);
    Hdr h;
    h.g = (const uint8_t*)ga;
    h.shift = (uint32_t)(ga & 15);
    // Stage only the header bytes the getters read: the last header the
    // record names ends by l4 + 20 (TCP) / inner + 40 / l3 + 40.
    uint32_t need = 22;
    if (ok) {
        const uint32_t l3 = r.eth_len + 40;
        need = l3 > need ? l3 : need;
        if (r.flags & ZP_F_IP_IN_IP) need = r.inner_off + 40 > need ? r.inner_off + 40 : need;
        if (r.flags & (ZP_F_TCP | ZP_F_UDP | ZP_F_ICMPV4 | ZP_F_ICMPV6))
            need = r.l4_off + 20 > need ? r.l4_off + 20 : need;
    }
    if (far) need = FX_WIN;             // eth_len / inner_off not known yet
    need = need < len ? need : len;
    h.wlen = need < FX_WIN - h.shift ? need : FX_WIN - h.shift;
    h.win = (const uint8_t*)&win[threadIdx.x];
    h.xc = make_uint4(0, 0, 0, 0);
    h.xi = ~0u;
    fx_stage(win, ga, len, h);          // [A & ~15, A + wlen), cooperatively (zp_win.h)

    if (!live) return;
    HdrReader rd{h};
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
    emit_columns(rd, r, ok, len, i, c);
}

extern "C" int zp_extract_columns_device(const uint8_t* arena, const uint64_t* offs,
                                         const uint32_t* lens, const zp_record* records,
                                         uint64_t n, void* const* cols, void* stream) {
    if (n == 0) return 0;
    if (!arena || !offs || !lens || !records || !cols) {
        snprintf(zp__errbuf(), 256, "zp_extract_columns_device: null pointer");
        return -1;
    }
    ColPtrs c;
    bool any = false;
    for (int k = 0; k < ZP_COL_COUNT; ++k) {
        c.p[k] = (uint8_t*)cols[k];
        any |= c.p[k] != nullptr;
    }
    if (!any) return 0;
    const uint64_t blocks = (n + FX_BLOCK - 1) / FX_BLOCK;
    if (blocks > 0x7FFFFFFFull) {
        snprintf(zp__errbuf(), 256, "zp_extract_columns_device: batch too large");
        return -1;
    }
    hipLaunchKernelGGL(zp_columns_kernel, dim3((unsigned)blocks), dim3(FX_BLOCK), 0,
                       (hipStream_t)stream, arena, offs, lens, records, n, c);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        snprintf(zp__errbuf(), 256, "zp_columns_kernel launch: %s", hipGetErrorString(e));
        return -2;
    }
    return 0;
}
