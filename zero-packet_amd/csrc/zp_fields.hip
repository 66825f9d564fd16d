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
#include "zp_colrec.h"                   // zp_cols.h, zp_win.h (FX_WIN, the staged window and its
                                         // reader) and the record decode

extern "C" char* zp__errbuf(void);

static const int kColWidth[ZP_COL_COUNT] = {
    6, 6, 2, 2, 2, 2, 1, 16, 16, 1, 1, 1, 4, 2, 1, 16, 16, 1, 1, 2, 2, 4, 4, 1, 2, 1, 1, 2, 4};

extern "C" int zp_col_width(int col) {
    return col >= 0 && col < ZP_COL_COUNT ? kColWidth[col] : 0;
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
    const bool far = fx_rec_decode(q, r);            // zp_colrec.h
    const bool ok = live && r.err == 0 && (r.flags & ZP_F_ETHERNET);
    const uint32_t len = ok ? lens[i] : 0u;
    const uintptr_t ga = (uintptr_t)arena + (ok ? offs[i] : 0);
    Hdr h;
    h.g = (const uint8_t*)ga;
    h.shift = (uint32_t)(ga & 15);
    // Stage only the header bytes the getters read (zp_colrec.h).
    uint32_t need = fx_rec_need(r, ok, far, true, true, true);
    need = need < len ? need : len;
    h.wlen = need < FX_WIN - h.shift ? need : FX_WIN - h.shift;
    h.win = (const uint8_t*)&win[threadIdx.x];
    h.xc = make_uint4(0, 0, 0, 0);
    h.xi = ~0u;
    fx_stage(win, ga, len, h);          // [A & ~15, A + wlen), cooperatively (zp_win.h)

    if (!live) return;
    HdrReader rd{h};
    fx_rec_finish(rd, r, ok, far);
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
