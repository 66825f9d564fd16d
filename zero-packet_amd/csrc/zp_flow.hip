// zp_flow.hip — flow table: group parsed frames by key on the device, with
// per-flow counters (include/zero_packet.h, zp_flow_aggregate_device).
//
// Six launches on the caller's stream (seven past ZP_SELECT_SCAN_FRAMES). In
// one launch workgroups talk to each other through agent-scope integer atomics
// only; whatever is written with plain stores is read in a later launch.
//   key     one lane per frame: the header window staged and the record
//           decoded as in zp_select_mark_terms_kernel, the key assembled in
//           registers by a col_values() sink (zp_cols.h), made canonical for
//           ZP_FLOW_BIDIR and hashed. A 48-B row {key, hash, TCP flags} per
//           frame goes to scratch. The same launch clears the table and the
//           header words the later launches add into.
//   insert  open addressing, linear probing, over T >= 2 min(max_flows, n)
//           slots {claim, first}. A slot is claimed by a CAS of the frame's
//           index; a frame that finds it claimed compares its key with the
//           claimant's row (written by the launch before) and moves on only if
//           they differ. Then atomicMin(first) and the slot into the frame's
//           row. Lanes of a wave that share the key of the wave's first keyed
//           lane go through that lane (heavy hitters: one probe per wave).
//   mark    a frame is its flow's head when first[slot] == i. Ballot words,
//           a count per 256-frame tile, the keyed frames and bytes.
//   scan    exclusive sums of the tile counts (two levels, as select's).
//   heads   head i with rank r < max_flows writes flows[r] = {key, first = i,
//           zeros}; r goes into the slot's claim word either way.
//   label   f = rank of the frame's slot; flow_of[i] = f; last, packets,
//           bytes and tcp_flags by atomics on flows[f], equal f of a wave
//           combined first. The first lane writes `count`.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/zero_packet.h"
#include "zp_colrec.h"

extern "C" char* zp__errbuf(void);

#define FL_BLOCK FX_BLOCK
#define FL_WAVES (FL_BLOCK / 64)
#define FL_PER 4                            // scan: tiles per lane
#define FL_SPAN (FL_BLOCK * FL_PER)         // scan: tiles per workgroup
#define FL_EMPTY 0xFFFFFFFFu                // a free slot's claim word
#define FL_ROW 12                           // dwords per row: key[10], hash -> slot, FL_KEYED | TCP flags
#define FL_KEYED 0x100u                     // a row's last dword: the frame is keyed
#define FL_CNT 64                           // header: spread of the keyed-frame / byte sums
#define FL_MAX_TABLE_FLOWS (1ull << 30)     // T = 2^31 slots at most: a slot number fits 32 bits

static_assert(ZP_SELECT_SCAN_FRAMES == (uint64_t)FL_SPAN * FL_BLOCK, "the scan span of zero_packet.h");
static_assert(sizeof(zp_flow_key) == 40 && sizeof(zp_flow_entry) == 64 && sizeof(zp_flow_opts) == 24,
              "zero_packet.h states the sizes");

// The head of scratch: what the launches add into across workgroups.
struct FlHdr {
    uint64_t cnt[FL_CNT][2];                // {keyed frames, keyed bytes}, summed by label
    uint64_t flows;                         // F (scan)
    uint32_t overflow;
    uint32_t pad[13];
};
static_assert(sizeof(FlHdr) == 1088, "a multiple of 16: the rows behind it are 16-B aligned");

typedef uint32_t FX_GLOBAL* fl_gu32;
typedef uint64_t FX_GLOBAL* fl_gu64;

__device__ __forceinline__ uint32_t fl_cas(uint32_t* p, uint32_t expect, uint32_t v) {
    __hip_atomic_compare_exchange_strong((fl_gu32)p, &expect, v, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_AGENT);
    return expect;
}
__device__ __forceinline__ void fl_min(uint32_t* p, uint32_t v) {
    __hip_atomic_fetch_min((fl_gu32)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void fl_max(uint32_t* p, uint32_t v) {
    __hip_atomic_fetch_max((fl_gu32)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void fl_add(uint32_t* p, uint32_t v) {
    __hip_atomic_fetch_add((fl_gu32)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void fl_or(uint32_t* p, uint32_t v) {
    __hip_atomic_fetch_or((fl_gu32)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void fl_add64(uint64_t* p, uint64_t v) {
    __hip_atomic_fetch_add((fl_gu64)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Sum of a u32 over the wave, exact in 64 bits (two 16-bit halves).
__device__ __forceinline__ uint64_t fl_wave_sum(uint32_t v) {
    uint32_t lo = v & 0xFFFFu, hi = v >> 16;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo += __shfl_xor(lo, o);
        hi += __shfl_xor(hi, o);
    }
    return ((uint64_t)hi << 16) + lo;
}

// col_values' sink that keeps the key's columns in registers. It starts from
// the all-zero value of every column.
struct FlowSink {
    uint4 src, dst;
    uint32_t sport, dport, l4p, ipv, tci, tflags;
    static constexpr bool kStore = false;
    static __device__ __forceinline__ bool l3() { return true; }
    static __device__ __forceinline__ bool inner() { return false; }
    static __device__ __forceinline__ bool l4() { return true; }
    template <class R>
    __device__ __forceinline__ void mac(int, R&, uint32_t) {}
    template <class R>
    __device__ __forceinline__ void addr(int col, R& rd, uint32_t x, bool v6) {   // as col_addr
        if (col != ZP_COL_SRC_ADDR && col != ZP_COL_DEST_ADDR) return;
        uint4 v;
        v.x = rd_le(rd, x, 4);
        v.y = v6 ? rd_le(rd, x + 4, 4) : 0u;
        v.z = v6 ? rd_le(rd, x + 8, 4) : 0u;
        v.w = v6 ? rd_le(rd, x + 12, 4) : 0u;
        if (col == ZP_COL_SRC_ADDR) src = v;
        else dst = v;
    }
    template <typename T>
    __device__ __forceinline__ void put(int col, T v) {
        if (col == ZP_COL_SRC_PORT) sport = (uint32_t)v;
        else if (col == ZP_COL_DEST_PORT) dport = (uint32_t)v;
        else if (col == ZP_COL_L4_PROTO) l4p = (uint32_t)v;
        else if (col == ZP_COL_IP_VERSION) ipv = (uint32_t)v;
        else if (col == ZP_COL_VLAN_TCI) tci = (uint32_t)v;
        else if (col == ZP_COL_TCP_FLAGS) tflags = (uint32_t)v;
    }
};

// An address as extracted (memory order in LE dwords) against another, by bytes.
__device__ __forceinline__ int fl_addr_cmp(const uint4& a, const uint4& b) {
    const uint32_t x[4] = {a.x, a.y, a.z, a.w}, y[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (x[k] != y[k]) return __builtin_bswap32(x[k]) < __builtin_bswap32(y[k]) ? -1 : 1;
    return 0;
}

__device__ __forceinline__ uint64_t fl_hash(const uint32_t* kw) {
    uint64_t h = 0x9E3779B97F4A7C15ull;
#pragma unroll
    for (int k = 0; k < 10; k += 2) {
        h ^= ((uint64_t)kw[k + 1] << 32) | kw[k];
        h *= 0xFF51AFD7ED558CCDull;
        h ^= h >> 32;
    }
    h *= 0xC4CEB9FE1A85EC53ull;
    return h ^ (h >> 29);
}

// ---- key ---------------------------------------------------------------------
// rows[i] = {key, masked hash folded to 32 bits, FL_KEYED | TCP flags}, or
// {.., ZP_FLOW_NONE, 0} for a frame that is not keyed (a hash can be any word,
// so the last dword says which). The grid also clears the table (claim =
// FL_EMPTY, first = ~0) and the header.
__global__ void __launch_bounds__(FL_BLOCK)
zp_flow_key_kernel(const uint8_t* __restrict__ arena, const uint64_t* __restrict__ offs,
                   const uint32_t* __restrict__ lens, const zp_record* __restrict__ recs,
                   uint64_t n, const uint64_t* __restrict__ mask, uint32_t key_flags,
                   uint64_t hash_mask, uint4* __restrict__ rows, uint64_t* __restrict__ table,
                   uint64_t slots, FlHdr* __restrict__ hdr) {
    __shared__ uint4 win[FX_CH * FX_BLOCK];
    const uint64_t i0 = (uint64_t)blockIdx.x * FX_BLOCK + threadIdx.x;
    for (uint64_t s = i0; s < slots; s += (uint64_t)gridDim.x * FX_BLOCK) table[s] = ~0ull;
    if (blockIdx.x == 0)
        for (uint32_t k = threadIdx.x; k < sizeof(FlHdr) / 8; k += FX_BLOCK) ((uint64_t*)hdr)[k] = 0;
    // Lanes past the batch stay for the cooperative staging.
    const bool live = i0 < n;
    const uint64_t i = live ? i0 : n - 1;
    zp_rec_full r;
    const zp_u32x2 q = *(const FX_GLOBAL zp_u32x2*)(recs + i);
    const bool far = fx_rec_decode(q, r);            // zp_colrec.h
    bool ok = live && r.err == 0 && (r.flags & ZP_F_ETHERNET) && (r.flags & (ZP_F_IPV4 | ZP_F_IPV6));
    if (mask) ok = ok && ((mask[i >> 6] >> (i & 63)) & 1u);
    const uint32_t len = ok ? lens[i] : 0u;          // a frame that is not keyed is not staged
    const uintptr_t ga = (uintptr_t)arena + (ok ? offs[i] : 0);
    FlowSink s;
    s.src = s.dst = make_uint4(0, 0, 0, 0);
    s.sport = s.dport = s.l4p = s.ipv = s.tci = s.tflags = 0;
    Hdr h;
    h.g = (const uint8_t*)ga;
    h.shift = (uint32_t)(ga & 15);
    uint32_t need = fx_rec_need(r, ok, far, true, false, true);
    need = need < len ? need : len;
    h.wlen = need < FX_WIN - h.shift ? need : FX_WIN - h.shift;
    h.win = (const uint8_t*)&win[threadIdx.x];
    h.xc = make_uint4(0, 0, 0, 0);
    h.xi = ~0u;
    fx_stage(win, ga, len, h);

    HdrReader rd{h};
    // Only the far form's eth_len is needed: the final next headers feed
    // ZP_COL_PROTOCOL and the ip_in_ip group, which the key does not hold.
    fx_rec_finish(rd, r, ok && far, far);
    col_values(rd, r, ok, len, s);
    if (!live) return;
    uint4* const row = rows + 3 * i0;
    if (!ok) {
        row[2] = make_uint4(0, 0, ZP_FLOW_NONE, 0);
        return;
    }
    if (!(key_flags & ZP_FLOW_PORTS)) s.sport = s.dport = 0;
    if (!(key_flags & ZP_FLOW_PROTO)) s.l4p = 0;
    const uint32_t vlan = (key_flags & ZP_FLOW_VLAN) ? s.tci & 0x0FFFu : 0u;
    if (key_flags & ZP_FLOW_BIDIR) {
        const int c = fl_addr_cmp(s.src, s.dst);
        if (c > 0 || (c == 0 && s.sport > s.dport)) {
            const uint4 a = s.src;
            s.src = s.dst;
            s.dst = a;
            const uint32_t p = s.sport;
            s.sport = s.dport;
            s.dport = p;
        }
    }
    const uint32_t kw[10] = {s.src.x, s.src.y, s.src.z, s.src.w, s.dst.x, s.dst.y, s.dst.z, s.dst.w,
                             s.sport | (s.dport << 16), s.l4p | (s.ipv << 8) | (vlan << 16)};
    const uint64_t hm = fl_hash(kw) & hash_mask;
    row[0] = s.src;
    row[1] = s.dst;
    row[2] = make_uint4(kw[8], kw[9], (uint32_t)hm ^ (uint32_t)(hm >> 32), FL_KEYED | s.tflags);
}

// ---- insert -------------------------------------------------------------------
// The slot of frame i's key: claimed by i, or claimed by a frame with the same
// key. ZP_FLOW_NONE (and the overflow word set) after a probe of every slot.
__device__ __forceinline__ uint32_t fl_probe(uint32_t* __restrict__ tab, uint32_t tmask,
                                             const uint4* __restrict__ rows, uint32_t i,
                                             const uint4& k0, const uint4& k1, uint32_t k8,
                                             uint32_t k9, uint32_t hash, FlHdr* hdr) {
    uint32_t s = hash & tmask;
    for (uint64_t p = 0; p <= tmask; ++p, s = (s + 1) & tmask) {
        const uint32_t c = fl_cas(&tab[2 * (uint64_t)s], FL_EMPTY, i);
        if (c != FL_EMPTY && c != i) {
            // the claimant's key: a row of the key launch
            const uint4* const o = rows + 3 * (uint64_t)c;
            const uint4 a = o[0], b = o[1];
            const uint2 e = *(const uint2*)(o + 2);
            if (a.x != k0.x || a.y != k0.y || a.z != k0.z || a.w != k0.w || b.x != k1.x ||
                b.y != k1.y || b.z != k1.z || b.w != k1.w || e.x != k8 || e.y != k9)
                continue;
        }
        fl_min(&tab[2 * (uint64_t)s + 1], i);
        return s;
    }
    fl_or(&hdr->overflow, 1u);
    return ZP_FLOW_NONE;
}

template <bool COMBINE>
__global__ void __launch_bounds__(FL_BLOCK)
zp_flow_insert_kernel(uint64_t n, uint4* __restrict__ rows, uint32_t* __restrict__ tab,
                      uint32_t tmask, FlHdr* __restrict__ hdr) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t i0 = (uint64_t)blockIdx.x * FL_BLOCK + threadIdx.x;
    const bool live = i0 < n;
    const uint64_t i = live ? i0 : n - 1;
    const uint4 k0 = rows[3 * i], k1 = rows[3 * i + 1], k2 = rows[3 * i + 2];
    const bool keyed = live && (k2.w & FL_KEYED);
    bool done = !keyed;
    uint32_t slot = ZP_FLOW_NONE;
    if (COMBINE) {
        // Lanes that hold the key of the first pending lane take that lane's
        // slot; its index is the smallest of them. Two rounds, and none after
        // a group of one: traffic of distinct keys pays one comparison.
        uint64_t rem = __ballot(!done);
        for (int round = 0; round < 2 && rem; ++round) {
            const int ld = __builtin_ctzll(rem);
            const uint32_t kw[10] = {k0.x, k0.y, k0.z, k0.w, k1.x, k1.y, k1.z, k1.w, k2.x, k2.y};
            bool same = !done;
#pragma unroll
            for (int k = 0; k < 10; ++k)
                same = same && kw[k] == (uint32_t)__builtin_amdgcn_readlane((int)kw[k], ld);
            const uint64_t g = __ballot(same);
            uint32_t s = ZP_FLOW_NONE;
            if ((int)lane == ld) s = fl_probe(tab, tmask, rows, (uint32_t)i, k0, k1, k2.x, k2.y, k2.z, hdr);
            s = (uint32_t)__builtin_amdgcn_readlane((int)s, ld);
            if (same) {
                slot = s;
                done = true;
            }
            rem &= ~g;
            if (__builtin_popcountll(g) == 1) break;
        }
    }
    if (!done) slot = fl_probe(tab, tmask, rows, (uint32_t)i, k0, k1, k2.x, k2.y, k2.z, hdr);
    if (keyed) ((uint32_t*)(rows + 3 * i))[10] = slot;   // over the hash: the row's slot from here on
}

// ---- mark ---------------------------------------------------------------------
__global__ void __launch_bounds__(FL_BLOCK)
zp_flow_mark_kernel(const uint32_t* __restrict__ lens, uint64_t n, const uint4* __restrict__ rows,
                    const uint32_t* __restrict__ tab, uint64_t* __restrict__ ballots,
                    uint32_t* __restrict__ part, FlHdr* __restrict__ hdr) {
    __shared__ uint64_t ws[FL_WAVES][3];
    const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const uint64_t i0 = (uint64_t)blockIdx.x * FL_BLOCK + threadIdx.x;
    const bool live = i0 < n;
    const uint64_t i = live ? i0 : n - 1;
    const uint32_t slot = ((const uint32_t*)(rows + 3 * i))[10];
    const bool keyed = live && slot != ZP_FLOW_NONE;
    const bool head = keyed && tab[2 * (uint64_t)slot + 1] == (uint32_t)i;
    const uint64_t b = __ballot(head), kb = __ballot(keyed);
    const uint64_t bytes = fl_wave_sum(keyed ? lens[i] : 0u);
    if (lane == 0) {
        if (live) ballots[i0 >> 6] = b;
        ws[wid][0] = (uint64_t)__builtin_popcountll(b);
        ws[wid][1] = (uint64_t)__builtin_popcountll(kb);
        ws[wid][2] = bytes;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t c = 0, k = 0, t = 0;
        for (int w = 0; w < FL_WAVES; ++w) {
            c += ws[w][0];
            k += ws[w][1];
            t += ws[w][2];
        }
        part[blockIdx.x] = (uint32_t)c;
        if (k) {
            fl_add64(&hdr->cnt[blockIdx.x % FL_CNT][0], k);
            fl_add64(&hdr->cnt[blockIdx.x % FL_CNT][1], t);
        }
    }
}

// ---- scan ---------------------------------------------------------------------
// Exclusive sums over `m` counts, in place; a workgroup covers FL_SPAN of
// them. `loop`: one workgroup walks the whole array with a carry (the second
// level). The total goes to tot[b] of workgroup b, and to *flows when this
// launch sees the whole array. Sums stay below 2^32 (n does).
__global__ void __launch_bounds__(FL_BLOCK)
zp_flow_scan_kernel(uint32_t* __restrict__ part, uint64_t m, uint32_t* __restrict__ tot,
                    uint64_t* __restrict__ flows, int loop) {
    __shared__ uint32_t ws[FL_WAVES];
    const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    uint32_t carry = 0;
    uint64_t first = loop ? 0 : (uint64_t)blockIdx.x * FL_SPAN;
    const uint64_t last = loop ? m : (first + FL_SPAN < m ? first + FL_SPAN : m);
    for (; first < last; first += FL_SPAN) {
        const uint64_t j0 = first + (uint64_t)threadIdx.x * FL_PER;
        uint32_t c[FL_PER], tc = 0;
#pragma unroll
        for (int k = 0; k < FL_PER; ++k) {
            c[k] = j0 + k < last ? part[j0 + k] : 0u;
            tc += c[k];
        }
        uint32_t ic = tc;                             // inclusive over the wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t u = __shfl_up(ic, o);
            if (lane >= (uint32_t)o) ic += u;
        }
        if (lane == 63) ws[wid] = ic;
        __syncthreads();
        uint32_t bc = carry, all = 0;
        for (int w = 0; w < FL_WAVES; ++w) {
            if (w < (int)wid) bc += ws[w];
            all += ws[w];
        }
        __syncthreads();                              // ws is reused by the next span
        bc += ic - tc;
#pragma unroll
        for (int k = 0; k < FL_PER; ++k) {
            if (j0 + k < last) part[j0 + k] = bc;
            bc += c[k];
        }
        carry += all;
    }
    if (threadIdx.x == 0) {
        if (tot) tot[blockIdx.x] = carry;
        if (flows) *flows = carry;
    }
}

// ---- heads --------------------------------------------------------------------
__global__ void __launch_bounds__(FL_BLOCK)
zp_flow_heads_kernel(uint64_t n, const uint4* __restrict__ rows, uint32_t* __restrict__ tab,
                     const uint64_t* __restrict__ ballots, const uint32_t* __restrict__ part,
                     const uint32_t* __restrict__ tot, uint64_t max_flows,
                     uint64_t* __restrict__ flows, FlHdr* __restrict__ hdr) {
    __shared__ uint32_t ws[FL_WAVES];
    const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const uint64_t tile = blockIdx.x;
    const uint64_t i = tile * FL_BLOCK + threadIdx.x;
    const uint64_t w0 = i - lane;                      // the wave's first frame
    const uint64_t b = w0 < n ? ballots[w0 >> 6] : 0;  // wave-uniform; bits at and past n are 0
    const bool head = (b >> lane) & 1u;
    const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32),
                                                     __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
    if (lane == 63) ws[wid] = (uint32_t)__builtin_popcountll(b);
    __syncthreads();
    uint32_t rank = part[tile] + below;
    if (tot) rank += tot[tile / FL_SPAN];
    for (int w = 0; w < (int)wid; ++w) rank += ws[w];
    if (!head) return;
    const uint4 k0 = rows[3 * i], k1 = rows[3 * i + 1], k2 = rows[3 * i + 2];
    tab[2 * (uint64_t)k2.z] = rank;                    // the claim word: the flow's number from here on
    if (rank >= max_flows) {
        fl_or(&hdr->overflow, 1u);
        return;
    }
    uint64_t* const e = flows + 8 * (uint64_t)rank;    // zp_flow_entry as eight 8-B words
    e[0] = ((uint64_t)k0.y << 32) | k0.x;
    e[1] = ((uint64_t)k0.w << 32) | k0.z;
    e[2] = ((uint64_t)k1.y << 32) | k1.x;
    e[3] = ((uint64_t)k1.w << 32) | k1.z;
    e[4] = ((uint64_t)k2.y << 32) | k2.x;
    e[5] = (uint32_t)i;                                // first = i, last = 0
    e[6] = 0;                                          // packets, tcp_flags, pad
    e[7] = 0;                                          // bytes
}

// ---- label --------------------------------------------------------------------
__device__ __forceinline__ void fl_contribute(uint64_t* flows, uint32_t f, uint32_t last,
                                              uint32_t packets, uint64_t bytes, uint32_t tflags) {
    uint32_t* const e = (uint32_t*)(flows + 8 * (uint64_t)f);
    fl_max(e + 11, last);
    fl_add(e + 12, packets);
    if (tflags) fl_or(e + 13, tflags);                 // tcp_flags: the word's low byte, pad above it
    fl_add64((uint64_t*)(e + 14), bytes);
}

template <bool COMBINE>
__global__ void __launch_bounds__(FL_BLOCK)
zp_flow_label_kernel(const uint32_t* __restrict__ lens, uint64_t n, const uint4* __restrict__ rows,
                     const uint32_t* __restrict__ tab, uint64_t max_flows,
                     uint32_t* __restrict__ flow_of, uint64_t* __restrict__ flows,
                     const FlHdr* __restrict__ hdr, uint64_t* __restrict__ count) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t i0 = (uint64_t)blockIdx.x * FL_BLOCK + threadIdx.x;
    if (i0 == 0) {
        uint64_t k = 0, t = 0;
        for (int c = 0; c < FL_CNT; ++c) {
            k += hdr->cnt[c][0];
            t += hdr->cnt[c][1];
        }
        count[0] = hdr->flows;
        count[1] = k;
        count[2] = t;
        count[3] = hdr->overflow || hdr->flows > max_flows;
    }
    const bool live = i0 < n;
    const uint64_t i = live ? i0 : n - 1;
    const uint2 st = *(const uint2*)((const uint32_t*)(rows + 3 * i) + 10);   // {slot, TCP flags}
    uint32_t f = ZP_FLOW_NONE;
    if (live && st.x != ZP_FLOW_NONE) f = tab[2 * (uint64_t)st.x];
    const bool valid = f != ZP_FLOW_NONE && f < max_flows;   // at and past max_flows: overflow
    if (live && flow_of) flow_of[i] = valid ? f : ZP_FLOW_NONE;
    const uint32_t len = valid ? lens[i] : 0u, tf = valid ? st.y & 0xFFu : 0u;
    bool done = !valid;
    if (COMBINE) {
        uint64_t rem = __ballot(!done);
        for (int round = 0; round < 2 && rem; ++round) {
            const int ld = __builtin_ctzll(rem);
            const bool same = !done && f == (uint32_t)__builtin_amdgcn_readlane((int)f, ld);
            const uint64_t g = __ballot(same);
            const uint32_t cnt = (uint32_t)__builtin_popcountll(g);
            if (cnt == 1) break;                       // distinct flows: every lane for itself
            const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)i,
                                                                    63 - __builtin_clzll(g));
            const uint64_t bytes = fl_wave_sum(same ? len : 0u);
            uint32_t fo = same ? tf : 0u;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) fo |= __shfl_xor(fo, o);
            if ((int)lane == ld) fl_contribute(flows, f, hi, cnt, bytes, fo);
            done = done || same;
            rem &= ~g;
        }
    }
    if (!done) fl_contribute(flows, f, (uint32_t)i, 1u, len, tf);
}

// ---- host ---------------------------------------------------------------------
static int fl_combine = 1;

// Test / measurement hook: in-wave combining of equal keys on (1) or off (0);
// returns the previous setting. Results are the same either way.
extern "C" int zp__flow_combine(int on) {
    const int was = fl_combine;
    if (on >= 0) fl_combine = on != 0;
    return was;
}

static uint64_t fl_tiles(uint64_t n) { return (n + FL_BLOCK - 1) / FL_BLOCK; }
static uint64_t fl_spans(uint64_t n) { return (fl_tiles(n) + FL_SPAN - 1) / FL_SPAN; }
static uint64_t fl_up16(uint64_t x) { return (x + 15) & ~15ull; }

// Slots: the first power of two >= 2 min(max_flows, n), at least 64. More
// than n flows cannot occur, so a larger max_flows needs no larger table.
static uint64_t fl_slots(uint64_t n, uint64_t max_flows) {
    uint64_t m = max_flows < n ? max_flows : n;
    if (m > FL_MAX_TABLE_FLOWS) m = FL_MAX_TABLE_FLOWS;
    uint64_t t = 64;
    while (t < 2 * m) t <<= 1;
    return t;
}

extern "C" uint64_t zp_flow_scratch_bytes(uint64_t n, uint64_t max_flows) {
    if (n >= (1ull << 32)) n = (1ull << 32) - 1;       // refused by the call
    return 16 + sizeof(FlHdr) + 4 * FL_ROW * n + fl_up16(8 * ((n + 63) / 64)) +
           fl_up16(4 * fl_tiles(n)) + fl_up16(4 * fl_spans(n)) + 8 * fl_slots(n, max_flows);
}

static int fl_fail(const char* what) {
    snprintf(zp__errbuf(), 256, "zp_flow_aggregate_device: %s", what);
    return -1;
}

static int fl_launched(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return 0;
    snprintf(zp__errbuf(), 256, "%s launch: %s", what, hipGetErrorString(e));
    return -2;
}

extern "C" int zp_flow_aggregate_device(const uint8_t* arena, const uint64_t* offs,
                                        const uint32_t* lens, const zp_record* records, uint64_t n,
                                        const zp_flow_opts* opts, const uint64_t* mask,
                                        uint32_t* flow_of, zp_flow_entry* flows, uint64_t* count,
                                        void* scratch, uint64_t scratch_bytes, void* stream) {
    if (!opts) return fl_fail("null opts");
    if (!count) return fl_fail("null count");
    if (opts->key_flags & ~(ZP_FLOW_PORTS | ZP_FLOW_PROTO | ZP_FLOW_VLAN | ZP_FLOW_BIDIR))
        return fl_fail("unknown key_flags bits");
    if (opts->pad) return fl_fail("pad must be 0");
    if (opts->max_flows == 0) return fl_fail("max_flows must not be 0");
    if ((uintptr_t)count & 7) return fl_fail("misaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        if (hipMemsetAsync(count, 0, 32, st) != hipSuccess) {
            snprintf(zp__errbuf(), 256, "zp_flow_aggregate_device: clearing count failed");
            return -2;
        }
        return 0;
    }
    if (!records) return fl_fail("null records");
    if (!lens) return fl_fail("null lens");
    if (!arena) return fl_fail("null arena");
    if (!offs) return fl_fail("null offs");
    if (!flows) return fl_fail("null flows");
    if (n >= (1ull << 32)) return fl_fail("frame indices are 32-bit: n must be below 2^32");
    if ((opts->max_flows < n ? opts->max_flows : n) > FL_MAX_TABLE_FLOWS)
        return fl_fail("batch too large: min(max_flows, n) above 2^30");
    if (!scratch || scratch_bytes < zp_flow_scratch_bytes(n, opts->max_flows))
        return fl_fail("scratch is null or below zp_flow_scratch_bytes(n, max_flows)");
    if (((uintptr_t)flows & 7) || ((uintptr_t)mask & 7) || ((uintptr_t)flow_of & 3))
        return fl_fail("misaligned pointer");
    const uint64_t tiles = fl_tiles(n), spans = fl_spans(n), slots = fl_slots(n, opts->max_flows);
    uint8_t* p = (uint8_t*)(((uintptr_t)scratch + 15) & ~(uintptr_t)15);
    FlHdr* const hdr = (FlHdr*)p;
    p += sizeof(FlHdr);
    uint4* const rows = (uint4*)p;
    p += 4 * FL_ROW * n;
    uint64_t* const ballots = (uint64_t*)p;
    p += fl_up16(8 * ((n + 63) / 64));
    uint32_t* const part = (uint32_t*)p;
    p += fl_up16(4 * tiles);
    uint32_t* const tot = (uint32_t*)p;
    p += fl_up16(4 * spans);
    uint32_t* const tab = (uint32_t*)p;
    const uint32_t tmask = (uint32_t)(slots - 1);
    const dim3 grid((unsigned)tiles), block(FL_BLOCK);
    int rc;
    hipLaunchKernelGGL(zp_flow_key_kernel, grid, block, 0, st, arena, offs, lens, records, n, mask,
                       opts->key_flags, opts->hash_mask, rows, (uint64_t*)tab, slots, hdr);
    if ((rc = fl_launched("zp_flow_key_kernel"))) return rc;
    if (fl_combine)
        hipLaunchKernelGGL(zp_flow_insert_kernel<true>, grid, block, 0, st, n, rows, tab, tmask, hdr);
    else
        hipLaunchKernelGGL(zp_flow_insert_kernel<false>, grid, block, 0, st, n, rows, tab, tmask, hdr);
    if ((rc = fl_launched("zp_flow_insert_kernel"))) return rc;
    hipLaunchKernelGGL(zp_flow_mark_kernel, grid, block, 0, st, lens, n, rows, tab, ballots, part, hdr);
    if ((rc = fl_launched("zp_flow_mark_kernel"))) return rc;
    if (spans == 1) {
        hipLaunchKernelGGL(zp_flow_scan_kernel, dim3(1), block, 0, st, part, tiles, (uint32_t*)nullptr,
                           &hdr->flows, 0);
    } else {
        hipLaunchKernelGGL(zp_flow_scan_kernel, dim3((unsigned)spans), block, 0, st, part, tiles, tot,
                           (uint64_t*)nullptr, 0);
        if ((rc = fl_launched("zp_flow_scan_kernel"))) return rc;
        hipLaunchKernelGGL(zp_flow_scan_kernel, dim3(1), block, 0, st, tot, spans, (uint32_t*)nullptr,
                           &hdr->flows, 1);
    }
    if ((rc = fl_launched("zp_flow_scan_kernel"))) return rc;
    hipLaunchKernelGGL(zp_flow_heads_kernel, grid, block, 0, st, n, rows, tab, ballots, part,
                       spans == 1 ? (const uint32_t*)nullptr : tot, opts->max_flows, (uint64_t*)flows,
                       hdr);
    if ((rc = fl_launched("zp_flow_heads_kernel"))) return rc;
    if (fl_combine)
        hipLaunchKernelGGL(zp_flow_label_kernel<true>, grid, block, 0, st, lens, n, rows, tab,
                           opts->max_flows, flow_of, (uint64_t*)flows, hdr, count);
    else
        hipLaunchKernelGGL(zp_flow_label_kernel<false>, grid, block, 0, st, lens, n, rows, tab,
                           opts->max_flows, flow_of, (uint64_t*)flows, hdr, count);
    return fl_launched("zp_flow_label_kernel");
}
