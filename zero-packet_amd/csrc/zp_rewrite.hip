// zp_rewrite.hip — batched header rewrite: columns written back into parsed
// frames (include/zero_packet.h, zp_rewrite_columns_device).
//
// The reference's XWriter setters over frames that already exist
// (EthernetWriter ethernet.rs:47-129, IPv4Writer ipv4.rs:46-126, IPv6Writer
// ipv6.rs:42-133, TcpWriter tcp.rs:37-129, UdpWriter udp.rs:37-71), driven by
// the zp_record the parse wrote: the record says where each header starts and
// which readers exist, the columns carry the new field values in the layout
// zp_extract_columns_device writes them.
//
// One lane per frame, 256 frames per workgroup, the header window staged as
// in zp_columns_kernel (zp_win.h). A frame the parse accepted has valid
// checksums, so both are updated from the changed words alone (zp_rewrite.h)
// and the payload is not read: per frame the header's one or two 128-B
// lines in, the written bytes out. The one exception is an L4 slice long
// enough for the reference's u32 sum to wrap (ZP_REWRITE_EXACT_L4_BYTES, IPv6
// jumbograms): its lane sums the new slice in full (rw_l4_exact).

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/zero_packet.h"
#include "zp_rewrite.h"
#include "zp_win.h"

extern "C" char* zp__errbuf(void);

static const char* const kColName[ZP_COL_COUNT] = {
    "DEST_MAC", "SRC_MAC", "ETHERTYPE", "VLAN_TCI", "VLAN_INNER_TCI", "ARP_OPER", "IP_VERSION",
    "SRC_ADDR", "DEST_ADDR", "PROTOCOL", "TTL", "TOS", "IP_ID", "IP_LEN", "INNER_VERSION",
    "INNER_SRC_ADDR", "INNER_DEST_ADDR", "INNER_PROTOCOL", "L4_PROTO", "SRC_PORT", "DEST_PORT",
    "TCP_SEQ", "TCP_ACK", "TCP_FLAGS", "TCP_WINDOW", "ICMP_TYPE", "ICMP_CODE", "L4_CHECKSUM",
    "PAYLOAD_OFF"};

extern "C" int zp_col_writable(int col) {
    switch (col) {
    case ZP_COL_DEST_MAC: case ZP_COL_SRC_MAC: case ZP_COL_VLAN_TCI: case ZP_COL_VLAN_INNER_TCI:
    case ZP_COL_SRC_ADDR: case ZP_COL_DEST_ADDR: case ZP_COL_TTL: case ZP_COL_TOS:
    case ZP_COL_IP_ID: case ZP_COL_SRC_PORT: case ZP_COL_DEST_PORT: case ZP_COL_TCP_SEQ:
    case ZP_COL_TCP_ACK: case ZP_COL_TCP_WINDOW:
        return 1;
    default:
        return 0;
    }
}

__global__ void __launch_bounds__(FX_BLOCK)
zp_rewrite_kernel(uint8_t* arena, const uint64_t* __restrict__ offs,
                  const uint32_t* __restrict__ lens, const zp_record* __restrict__ recs,
                  uint64_t n, ColPtrs c) {
    __shared__ uint4 win[FX_CH * FX_BLOCK];
    const uint64_t i0 = (uint64_t)blockIdx.x * FX_BLOCK + threadIdx.x;
    // Lanes past the batch stay for the cooperative staging (ds_bpermute reads
    // every lane); they load and store nothing.
    const bool live = i0 < n;
    const uint64_t i = live ? i0 : n - 1;
    // the 8-B record as zp_columns_kernel decodes it (include/zero_packet.h)
    static_assert(sizeof(zp_record) == 8, "one 8-B load per record");
    const zp_u32x2 q = *(const FX_GLOBAL zp_u32x2*)(recs + i);
    const uint32_t flags = q.x & ZP_F_MASK;
    // far-L4 form: offs holds the whole L4 offset, the Ethernet header length
    // is read from the frame after the staging
    const bool far = ((q.x >> 24) & 3u) == ZP_ETH_CODE_FAR;
    uint32_t hl = far ? 22u : 14u + 4u * ((q.x >> 24) & 3u);
    const uint32_t l4 = far ? q.y : q.y & ZP_L4_NEAR_MAX;
    const bool ok = live && (q.x >> 26) == 0 && (flags & ZP_F_ETHERNET);
    const uint32_t len = ok ? lens[i] : 0u;
    const uintptr_t ga = (uintptr_t)arena + (ok ? offs[i] : 0);
    Hdr h;
    h.g = (const uint8_t*)ga;
    h.shift = (uint32_t)(ga & 15);
    // Stage the header bytes the setters and the two checksums touch: the
    // outer IP header ends by l3 + 40, the L4 fields by l4 + 20 (TCP).
    uint32_t need = 22;
    if (ok) {
        need = hl + 40;
        if (flags & (ZP_F_TCP | ZP_F_UDP | ZP_F_ICMPV4 | ZP_F_ICMPV6))
            need = l4 + 20 > need ? l4 + 20 : need;
    }
    if (far) need = FX_WIN;
    need = need < len ? need : len;
    h.wlen = need < FX_WIN - h.shift ? need : FX_WIN - h.shift;
    h.win = (const uint8_t*)&win[threadIdx.x];
    h.xc = make_uint4(0, 0, 0, 0);
    h.xi = ~0u;
    fx_stage(win, ga, len, h);

    if (!ok || len < 14) return;
    HdrReader rd{h};
    if (far) {
        const uint32_t t0 = rd16(rd, 12u);                              // ethernet.rs:155-179
        hl = t0 == 0x8100 ? 18u : t0 == 0x88A8 ? 22u : 14u;
    }
    if (len < hl) return;
    rewrite_frame(rd, (FX_GLOBAL uint8_t*)ga, flags, hl, l4, len, i, c);
}

extern "C" int zp_rewrite_columns_device(uint8_t* arena, const uint64_t* offs,
                                         const uint32_t* lens, const zp_record* records,
                                         uint64_t n, const void* const* cols, void* stream) {
    ColPtrs c;
    bool any = false;
    for (int k = 0; k < ZP_COL_COUNT; ++k) {
        c.p[k] = cols ? (uint8_t*)cols[k] : nullptr;
        if (c.p[k] && !zp_col_writable(k)) {
            snprintf(zp__errbuf(), 256, "zp_rewrite_columns_device: column %d (ZP_COL_%s) is not "
                     "writable", k, kColName[k]);
            return -1;
        }
        any |= c.p[k] != nullptr;
    }
    if (n == 0 || !any) return 0;
    if (!arena || !offs || !lens || !records) {
        snprintf(zp__errbuf(), 256, "zp_rewrite_columns_device: null pointer");
        return -1;
    }
    const uint64_t blocks = (n + FX_BLOCK - 1) / FX_BLOCK;
    if (blocks > 0x7FFFFFFFull) {
        snprintf(zp__errbuf(), 256, "zp_rewrite_columns_device: batch too large");
        return -1;
    }
    hipLaunchKernelGGL(zp_rewrite_kernel, dim3((unsigned)blocks), dim3(FX_BLOCK), 0,
                       (hipStream_t)stream, arena, offs, lens, records, n, c);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        snprintf(zp__errbuf(), 256, "zp_rewrite_kernel launch: %s", hipGetErrorString(e));
        return -2;
    }
    return 0;
}
