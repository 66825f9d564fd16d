// zp_route.hip — route: longest-prefix match of a frame's outer source or
// destination address against a compiled prefix table (include/zero_packet.h,
// zp_route_device; the table and the walk: zp_route.h, zp_route_tab.c).
//
// One launch: one lane per frame, tiles of FX_BLOCK frames. A lane loads its
// record, and for a frame that is routed (no error, an outer IP reader, its
// bit of `only`) the header window is staged as far as the outer IP header
// reaches (zp_win.h, zp_colrec.h) and col_values() (zp_cols.h) hands
// ip_version and the chosen address to RouteSink. The walk is a chain of
// dependent 4-B gathers with per-lane addresses (vector loads): the roots in
// L2, deeper nodes wherever the table's size puts them; the waves of a CU
// hide one another's chains. The grid is sized to fill the device once and a
// workgroup walks several tiles. value_of is stored per lane, a mask word per
// wave by its first lane.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/zero_packet.h"
#include "zp_colrec.h"
#include "zp_route.h"

extern "C" char* zp__errbuf(void);

#define RT_BLOCK FX_BLOCK
// Workgroups one CU holds: 160 KiB of LDS over the 28 KiB window.
#define RT_WG_PER_CU 5

// col_values' sink: ip_version and one of the two outer addresses. It starts
// from the all-zero value of both.
struct RouteSink {
    int col;
    uint4 a;
    uint32_t ipv;
    static constexpr bool kStore = false;
    static __device__ __forceinline__ bool l3() { return true; }
    static __device__ __forceinline__ bool inner() { return false; }
    static __device__ __forceinline__ bool l4() { return false; }
    template <class R>
    __device__ __forceinline__ void mac(int, R&, uint32_t) {}
    template <class R>
    __device__ __forceinline__ void addr(int c, R& rd, uint32_t x, bool v6) {   // as col_addr
        if (c != col) return;
        a.x = rd_le(rd, x, 4);
        a.y = v6 ? rd_le(rd, x + 4, 4) : 0u;
        a.z = v6 ? rd_le(rd, x + 8, 4) : 0u;
        a.w = v6 ? rd_le(rd, x + 12, 4) : 0u;
    }
    template <typename T>
    __device__ __forceinline__ void put(int c, T v) {
        if (c == ZP_COL_IP_VERSION) ipv = (uint32_t)v;
    }
};

__global__ void __launch_bounds__(RT_BLOCK, RT_WG_PER_CU)
zp_route_kernel(const uint8_t* __restrict__ arena, const uint64_t* __restrict__ offs,
                const uint32_t* __restrict__ lens, const zp_record* __restrict__ recs, uint64_t n,
                const uint32_t* __restrict__ table, uint64_t table_bytes, int col,
                const uint64_t* __restrict__ only, uint32_t* __restrict__ value_of,
                uint64_t* __restrict__ mask, uint64_t* __restrict__ status) {
    __shared__ uint4 win[FX_CH * FX_BLOCK];
    // The header first: nothing behind it is read unless it is this table's.
    const bool good = rt_header_ok(table, table_bytes);
    if (blockIdx.x == 0 && threadIdx.x == 0) *status = good ? 0 : 1;
    if (!good || n == 0) return;                       // uniform over the grid
    const uint32_t nodes = table[RT_H_NODES];
    const uint32_t lane = threadIdx.x & 63;

    const uint64_t ntiles = (n + RT_BLOCK - 1) / RT_BLOCK;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        // Lanes past the batch stay for the cooperative staging and the ballot.
        const uint64_t i0 = tile * RT_BLOCK + threadIdx.x;
        const bool live = i0 < n;
        const uint64_t i = live ? i0 : n - 1;
        zp_rec_full r;
        const zp_u32x2 q = *(const FX_GLOBAL zp_u32x2*)(recs + i);
        const bool far = fx_rec_decode(q, r);          // zp_colrec.h
        bool ok = live && r.err == 0 && (r.flags & ZP_F_ETHERNET) &&
            (r.flags & (ZP_F_IPV4 | ZP_F_IPV6));
        if (only) ok = ok && ((only[i >> 6] >> (i & 63)) & 1u);
        const uint32_t len = ok ? lens[i] : 0u;        // a frame that is not routed is not staged
        const uintptr_t ga = (uintptr_t)arena + (ok ? offs[i] : 0);
        RouteSink s;
        s.col = col;
        s.a = make_uint4(0, 0, 0, 0);
        s.ipv = 0;
        Hdr h;
        h.g = (const uint8_t*)ga;
        h.shift = (uint32_t)(ga & 15);
        uint32_t need = fx_rec_need(r, ok, far, true, false, false);   // the outer IP header
        need = need < len ? need : len;
        h.wlen = need < FX_WIN - h.shift ? need : FX_WIN - h.shift;
        h.win = (const uint8_t*)&win[threadIdx.x];
        h.xc = make_uint4(0, 0, 0, 0);
        h.xi = ~0u;
        fx_stage(win, ga, len, h);
        HdrReader rd{h};
        // Only the far form's eth_len is needed: the final next headers feed
        // ZP_COL_PROTOCOL and the ip_in_ip group, which are not read here.
        fx_rec_finish(rd, r, ok && far, far);
        col_values(rd, r, ok, len, s);
        // the next tile's staging must not overtake this tile's reads of the window
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const uint32_t a[4] = {s.a.x, s.a.y, s.a.z, s.a.w};
        const uint32_t value = ok ? rt_lookup(table, nodes, a, s.ipv) : ZP_ROUTE_NONE;
        if (live && value_of) value_of[i0] = value;
        if (mask) {
            const uint64_t b = __ballot(live && value != ZP_ROUTE_NONE);
            if (lane == 0 && live) mask[i0 >> 6] = b;  // i0: the wave's first frame
        }
    }
}

// ---- host ------------------------------------------------------------------
static int rt_compute_units() {
    static int cus = 0;                                // one kind of device per process
    if (cus == 0) {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0)
            v = 256;
        cus = v;
    }
    return cus;
}

static int rt_fail(const char* what) {
    snprintf(zp__errbuf(), 256, "zp_route_device: %s", what);
    return -1;
}

extern "C" int zp_route_device(const uint8_t* arena, const uint64_t* offs, const uint32_t* lens,
                               const zp_record* records, uint64_t n, const void* table,
                               uint64_t table_bytes, int col, const uint64_t* only,
                               uint32_t* value_of, uint64_t* mask, uint64_t* status, void* stream) {
    if (!records) return rt_fail("null records");
    if (!table) return rt_fail("null table");
    if (!status) return rt_fail("null status");
    if (col != ZP_COL_DEST_ADDR && col != ZP_COL_SRC_ADDR)
        return rt_fail("col must be ZP_COL_DEST_ADDR or ZP_COL_SRC_ADDR");
    if (!arena || !offs || !lens) return rt_fail("route reads frames: it needs arena, offs and lens");
    if (n >= (1ull << 32)) return rt_fail("n must be below 2^32");
    if (table_bytes < rt_bytes(0)) return rt_fail("table_bytes below an empty table's");
    if (((uintptr_t)table & 7) || ((uintptr_t)only & 7) || ((uintptr_t)mask & 7) ||
        ((uintptr_t)status & 7) || ((uintptr_t)value_of & 3))
        return rt_fail("misaligned pointer");
    if (mask && only) {
        const uintptr_t words = 8 * (uintptr_t)((n + 63) / 64), m = (uintptr_t)mask, o = (uintptr_t)only;
        if (m < o + words && o < m + words) return rt_fail("mask overlaps only");
    }
    uint64_t blocks = n ? (n + RT_BLOCK - 1) / RT_BLOCK : 1;         // n == 0: status only
    // as many workgroups as the device holds at once, each walking several tiles
    const uint64_t fill = (uint64_t)rt_compute_units() * RT_WG_PER_CU;
    if (blocks > fill) blocks = fill;
    hipLaunchKernelGGL(zp_route_kernel, dim3((unsigned)blocks), dim3(RT_BLOCK), 0,
                       (hipStream_t)stream, arena, offs, lens, records, n, (const uint32_t*)table,
                       table_bytes, col, only, value_of, mask, status);
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return 0;
    snprintf(zp__errbuf(), 256, "zp_route_kernel launch: %s", hipGetErrorString(e));
    return -2;
}
