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
// The persistent table (zp_flow_update_device and its two companions) is the
// second half of the file; it runs the key, mark and scan kernels as their
// TABLE instantiations.

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
    uint32_t refused;                       // table update: frames of refused keys (label)
    uint32_t pad[12];
};
static_assert(sizeof(FlHdr) == 1088, "a multiple of 16: the rows behind it are 16-B aligned");

typedef uint32_t FX_GLOBAL* fl_gu32;
typedef uint64_t FX_GLOBAL* fl_gu64;

// The head of a persistent table's block; the slots (one dword each) follow.
struct FlTable {
    uint64_t magic, sig;                    // FL_MAGIC and a signature of the opts the table was made with
    uint64_t flows, epoch;                  // F and the number of updates completed
    uint64_t pad[4];
};
static_assert(sizeof(FlTable) == 64, "zero_packet.h states the header's size");
#define FL_MAGIC 0x31304C4654505A00ull      // "\0ZPTFL01"
#define FL_TAG 0x80000000u                  // a row's slot word: a flow number of the persistent table

// A launch on a persistent table goes on only when the header is the one
// `sig` was made from: two scalar loads, the same for every wave.
__device__ __forceinline__ bool fl_table_ok(const FlTable* t, uint64_t sig) {
    return t->magic == FL_MAGIC && t->sig == sig;
}

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

__host__ __device__ __forceinline__ uint64_t fl_hash(const uint32_t* kw) {
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

// The row's hash word: the masked hash folded to 32 bits.
__device__ __forceinline__ uint32_t fl_hash32(const uint32_t* kw, uint64_t hash_mask) {
    const uint64_t hm = fl_hash(kw) & hash_mask;
    return (uint32_t)hm ^ (uint32_t)(hm >> 32);
}

// ---- key ---------------------------------------------------------------------
// rows[i] = {key, masked hash folded to 32 bits, FL_KEYED | TCP flags}, or
// {.., ZP_FLOW_NONE, 0} for a frame that is not keyed (a hash can be any word,
// so the last dword says which). The grid also clears the table (claim =
// FL_EMPTY, first = ~0) and the header. TABLE: a launch of zp_flow_update_device,
// which does nothing unless `ptab` is the table `sig` describes.
template <bool TABLE>
__global__ void __launch_bounds__(FL_BLOCK)
zp_flow_key_kernel(const uint8_t* __restrict__ arena, const uint64_t* __restrict__ offs,
                   const uint32_t* __restrict__ lens, const zp_record* __restrict__ recs,
                   uint64_t n, const uint64_t* __restrict__ mask, uint32_t key_flags,
                   uint64_t hash_mask, uint4* __restrict__ rows, uint64_t* __restrict__ table,
                   uint64_t slots, FlHdr* __restrict__ hdr, const FlTable* __restrict__ ptab,
                   uint64_t sig) {
    __shared__ uint4 win[FX_CH * FX_BLOCK];
    if (TABLE && !fl_table_ok(ptab, sig)) return;
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
    row[0] = s.src;
    row[1] = s.dst;
    row[2] = make_uint4(kw[8], kw[9], fl_hash32(kw, hash_mask), FL_KEYED | s.tflags);
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
// TABLE: a frame whose slot word carries FL_TAG belongs to an established flow
// and is no head.
template <bool TABLE>
__global__ void __launch_bounds__(FL_BLOCK)
zp_flow_mark_kernel(const uint32_t* __restrict__ lens, uint64_t n, const uint4* __restrict__ rows,
                    const uint32_t* __restrict__ tab, uint64_t* __restrict__ ballots,
                    uint32_t* __restrict__ part, FlHdr* __restrict__ hdr,
                    const FlTable* __restrict__ ptab, uint64_t sig) {
    __shared__ uint64_t ws[FL_WAVES][3];
    if (TABLE && !fl_table_ok(ptab, sig)) return;
    const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const uint64_t i0 = (uint64_t)blockIdx.x * FL_BLOCK + threadIdx.x;
    const bool live = i0 < n;
    const uint64_t i = live ? i0 : n - 1;
    const uint32_t slot = ((const uint32_t*)(rows + 3 * i))[10];
    const bool keyed = live && slot != ZP_FLOW_NONE;
    const bool head = keyed && !(TABLE && (slot & FL_TAG)) && tab[2 * (uint64_t)slot + 1] == (uint32_t)i;
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
template <bool TABLE>
__global__ void __launch_bounds__(FL_BLOCK)
zp_flow_scan_kernel(uint32_t* __restrict__ part, uint64_t m, uint32_t* __restrict__ tot,
                    uint64_t* __restrict__ flows, int loop, const FlTable* __restrict__ ptab,
                    uint64_t sig) {
    __shared__ uint32_t ws[FL_WAVES];
    if (TABLE && !fl_table_ok(ptab, sig)) return;
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
    const FlTable* const none = nullptr;
    hipLaunchKernelGGL(zp_flow_key_kernel<false>, grid, block, 0, st, arena, offs, lens, records, n, mask,
                       opts->key_flags, opts->hash_mask, rows, (uint64_t*)tab, slots, hdr, none, 0ull);
    if ((rc = fl_launched("zp_flow_key_kernel"))) return rc;
    if (fl_combine)
        hipLaunchKernelGGL(zp_flow_insert_kernel<true>, grid, block, 0, st, n, rows, tab, tmask, hdr);
    else
        hipLaunchKernelGGL(zp_flow_insert_kernel<false>, grid, block, 0, st, n, rows, tab, tmask, hdr);
    if ((rc = fl_launched("zp_flow_insert_kernel"))) return rc;
    hipLaunchKernelGGL(zp_flow_mark_kernel<false>, grid, block, 0, st, lens, n, rows, tab, ballots, part,
                       hdr, none, 0ull);
    if ((rc = fl_launched("zp_flow_mark_kernel"))) return rc;
    if (spans == 1) {
        hipLaunchKernelGGL(zp_flow_scan_kernel<false>, dim3(1), block, 0, st, part, tiles,
                           (uint32_t*)nullptr, &hdr->flows, 0, none, 0ull);
    } else {
        hipLaunchKernelGGL(zp_flow_scan_kernel<false>, dim3((unsigned)spans), block, 0, st, part, tiles,
                           tot, (uint64_t*)nullptr, 0, none, 0ull);
        if ((rc = fl_launched("zp_flow_scan_kernel"))) return rc;
        hipLaunchKernelGGL(zp_flow_scan_kernel<false>, dim3(1), block, 0, st, tot, spans,
                           (uint32_t*)nullptr, &hdr->flows, 1, none, 0ull);
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

// ==== persistent table ===========================================================
// zp_flow_table_init_device / zp_flow_update_device / zp_flow_retire_device
// (include/zero_packet.h). The table block is a FlTable and T_P slots of one
// dword: FL_EMPTY or a flow number, whose key is flows[number].key. T_P >= 2
// max_flows, nothing is deleted between rebuilds, so a lookup misses at the
// first empty slot.
//
// An update is aggregate's sequence with the table in front of it. What a
// launch reads with plain loads was written by an earlier launch:
//   key     as above (rows, the transient table and the scratch header cleared).
//   find    reads P and flows[id].key (written by an earlier call's admit or
//           copy-back) and the rows (key). A hit puts FL_TAG | id into the row's
//           slot word, which only its own lane reads again. A miss goes through
//           fl_probe: CAS / min on the transient table, claimants' rows by plain
//           loads of words 0-9, which this launch does not write.
//   mark    reads the slot words (find) and first[] (find's atomicMin).
//   scan    reads the tile counts (mark).
//   admit   reads ballots, sums, rows; the head of rank r writes flows[F0 + r]
//           with plain stores (nobody reads flows here), claims a P slot by CAS
//           (nobody loads P here) and writes the id, or ZP_FLOW_NONE, into the
//           transient claim word, which no other lane of this launch touches.
//   label   reads the slot words (find), the claim words (admit) and adds into
//           flows[id] by atomics only; words 10-15 of an entry are never loaded.
//   finish  one lane: reads the sums (mark, scan, label), writes `count` and the
//           header's F and epoch, which every earlier launch read.
// F0 and E are the header's words as the call before left them.

struct FlRetHdr {
    uint64_t flows;                         // F' (scan)
    uint64_t pad;
};

__device__ __forceinline__ void fl_or64(uint64_t* p, uint64_t v) {
    __hip_atomic_fetch_or((fl_gu64)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ uint64_t fl_min64(uint64_t a, uint64_t b) { return a < b ? a : b; }

// The number of the key in P, or ZP_FLOW_NONE. Plain loads: P and the keys it
// points to are not written in the launch that looks up.
__device__ __forceinline__ uint32_t fl_find(const uint32_t* __restrict__ P, uint32_t pmask,
                                            const uint64_t* __restrict__ flows, uint64_t max_flows,
                                            const uint4& k0, const uint4& k1, uint32_t k8, uint32_t k9,
                                            uint32_t hash) {
    uint32_t s = hash & pmask;
    for (uint64_t p = 0; p <= pmask; ++p, s = (s + 1) & pmask) {
        const uint32_t id = P[s];
        if (id >= max_flows) return ZP_FLOW_NONE;      // FL_EMPTY (or not a table of ours)
        const uint4* const o = (const uint4*)(flows + 8 * (uint64_t)id);
        const uint4 a = o[0], b = o[1];
        const uint2 e = *(const uint2*)(o + 2);
        if (a.x == k0.x && a.y == k0.y && a.z == k0.z && a.w == k0.w && b.x == k1.x && b.y == k1.y &&
            b.z == k1.z && b.w == k1.w && e.x == k8 && e.y == k9)
            return id;
    }
    return ZP_FLOW_NONE;
}

// Puts `id` into the first empty slot from hash & pmask on. The keys inserted
// are pairwise distinct and not in P, so none is compared.
__device__ __forceinline__ void fl_claim(uint32_t* P, uint32_t pmask, uint32_t hash, uint32_t id) {
    uint32_t s = hash & pmask;
    for (uint64_t p = 0; p <= pmask; ++p, s = (s + 1) & pmask)
        if (fl_cas(&P[s], FL_EMPTY, id) == FL_EMPTY) return;
}

// A lane's rank among the set bits of the ballots: the tile's exclusive sum,
// the waves before this one and the lanes below. All lanes of the workgroup
// call it.
__device__ __forceinline__ uint32_t fl_rank(uint64_t b, uint32_t* ws, const uint32_t* part,
                                            const uint32_t* tot, uint64_t tile) {
    const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32),
                                                     __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
    if (lane == 63) ws[wid] = (uint32_t)__builtin_popcountll(b);
    __syncthreads();
    uint32_t rank = part[tile] + below;
    if (tot) rank += tot[tile / FL_SPAN];
    for (int w = 0; w < (int)wid; ++w) rank += ws[w];
    return rank;
}

// ---- init ----------------------------------------------------------------------
__global__ void __launch_bounds__(FL_BLOCK)
zp_flow_table_init_kernel(FlTable* __restrict__ t, uint64_t sig, uint64_t slots) {
    const uint64_t g = (uint64_t)blockIdx.x * FL_BLOCK + threadIdx.x;
    if (g < slots) ((uint32_t*)(t + 1))[g] = FL_EMPTY;
    if (g < sizeof(FlTable) / 8) {
        const uint64_t v = g == 0 ? FL_MAGIC : g == 1 ? sig : 0ull;
        ((uint64_t*)t)[g] = v;
    }
}

// ---- find + insert ---------------------------------------------------------------
// The slot word of frame i's row: FL_TAG | id for a key of the table, else its
// slot in the transient table (fl_probe).
__device__ __forceinline__ uint32_t fl_locate(const uint32_t* __restrict__ P, uint32_t pmask,
                                              const uint64_t* __restrict__ flows, uint64_t max_flows,
                                              bool lookup, uint32_t* __restrict__ tab, uint32_t tmask,
                                              const uint4* __restrict__ rows, uint32_t i, const uint4& k0,
                                              const uint4& k1, const uint4& k2, FlHdr* hdr) {
    if (lookup) {
        const uint32_t id = fl_find(P, pmask, flows, max_flows, k0, k1, k2.x, k2.y, k2.z);
        if (id != ZP_FLOW_NONE) return FL_TAG | id;
    }
    return fl_probe(tab, tmask, rows, i, k0, k1, k2.x, k2.y, k2.z, hdr);
}

template <bool COMBINE>
__global__ void __launch_bounds__(FL_BLOCK)
zp_flow_find_kernel(uint64_t n, uint4* __restrict__ rows, uint32_t* __restrict__ tab, uint32_t tmask,
                    FlHdr* __restrict__ hdr, const FlTable* __restrict__ ptab, uint64_t sig,
                    uint32_t pmask, const uint64_t* __restrict__ flows, uint64_t max_flows) {
    if (!fl_table_ok(ptab, sig)) return;
    const uint32_t* const P = (const uint32_t*)(ptab + 1);
    const bool lookup = ptab->flows != 0;              // an empty table: every key is new
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t i0 = (uint64_t)blockIdx.x * FL_BLOCK + threadIdx.x;
    const bool live = i0 < n;
    const uint64_t i = live ? i0 : n - 1;
    const uint4 k0 = rows[3 * i], k1 = rows[3 * i + 1], k2 = rows[3 * i + 2];
    const bool keyed = live && (k2.w & FL_KEYED);
    bool done = !keyed;
    uint32_t slot = ZP_FLOW_NONE;
    if (COMBINE) {                                     // as zp_flow_insert_kernel
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
            if ((int)lane == ld)
                s = fl_locate(P, pmask, flows, max_flows, lookup, tab, tmask, rows, (uint32_t)i, k0, k1,
                              k2, hdr);
            s = (uint32_t)__builtin_amdgcn_readlane((int)s, ld);
            if (same) {
                slot = s;
                done = true;
            }
            rem &= ~g;
            if (__builtin_popcountll(g) == 1) break;
        }
    }
    if (!done)
        slot = fl_locate(P, pmask, flows, max_flows, lookup, tab, tmask, rows, (uint32_t)i, k0, k1, k2, hdr);
    if (keyed) ((uint32_t*)(rows + 3 * i))[10] = slot;
}

// ---- admit ---------------------------------------------------------------------
__global__ void __launch_bounds__(FL_BLOCK)
zp_flow_admit_kernel(uint64_t n, const uint4* __restrict__ rows, uint32_t* __restrict__ tab,
                     const uint64_t* __restrict__ ballots, const uint32_t* __restrict__ part,
                     const uint32_t* __restrict__ tot, uint64_t max_flows, uint64_t hash_mask,
                     uint64_t* __restrict__ flows, FlTable* __restrict__ ptab, uint64_t sig,
                     uint32_t pmask) {
    __shared__ uint32_t ws[FL_WAVES];
    if (!fl_table_ok(ptab, sig)) return;
    const uint64_t f0 = fl_min64(ptab->flows, max_flows);
    const uint32_t epoch = (uint32_t)ptab->epoch;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t tile = blockIdx.x;
    const uint64_t i = tile * FL_BLOCK + threadIdx.x;
    const uint64_t w0 = i - lane;
    const uint64_t b = w0 < n ? ballots[w0 >> 6] : 0;  // wave-uniform; bits at and past n are 0
    const bool head = (b >> lane) & 1u;
    const uint32_t rank = fl_rank(b, ws, part, tot, tile);
    if (!head) return;
    const uint4 k0 = rows[3 * i], k1 = rows[3 * i + 1], k2 = rows[3 * i + 2];
    const uint64_t id = f0 + rank;
    if (id >= max_flows) {                             // refused: nothing of the key enters the table
        tab[2 * (uint64_t)k2.z] = ZP_FLOW_NONE;
        return;
    }
    tab[2 * (uint64_t)k2.z] = (uint32_t)id;            // the claim word: the flow's number from here on
    uint64_t* const e = flows + 8 * id;                // zp_flow_state as eight 8-B words
    e[0] = ((uint64_t)k0.y << 32) | k0.x;
    e[1] = ((uint64_t)k0.w << 32) | k0.z;
    e[2] = ((uint64_t)k1.y << 32) | k1.x;
    e[3] = ((uint64_t)k1.w << 32) | k1.z;
    e[4] = ((uint64_t)k2.y << 32) | k2.x;
    e[5] = ((uint64_t)epoch << 32) | epoch;            // first_epoch, last_epoch
    e[6] = 0;                                          // packets, TCP flags
    e[7] = 0;                                          // bytes
    const uint32_t kw[10] = {k0.x, k0.y, k0.z, k0.w, k1.x, k1.y, k1.z, k1.w, k2.x, k2.y};
    fl_claim((uint32_t*)(ptab + 1), pmask, fl_hash32(kw, hash_mask), (uint32_t)id);
}

// ---- label (table) ---------------------------------------------------------------
__device__ __forceinline__ void fl_state_add(uint64_t* flows, uint32_t f, uint32_t epoch,
                                             uint32_t packets, uint64_t bytes, uint32_t tflags) {
    uint64_t* const e = flows + 8 * (uint64_t)f;
    fl_max((uint32_t*)e + 11, epoch);                  // last_epoch
    fl_add64(e + 6, packets);
    if (tflags) fl_or64(e + 6, (uint64_t)tflags << 56);
    fl_add64(e + 7, bytes);
}

template <bool COMBINE>
__global__ void __launch_bounds__(FL_BLOCK)
zp_flow_table_label_kernel(const uint32_t* __restrict__ lens, uint64_t n, const uint4* __restrict__ rows,
                           const uint32_t* __restrict__ tab, uint32_t* __restrict__ flow_of,
                           uint64_t* __restrict__ flows, FlHdr* __restrict__ hdr,
                           const FlTable* __restrict__ ptab, uint64_t sig, uint64_t max_flows) {
    if (!fl_table_ok(ptab, sig)) return;
    const uint32_t epoch = (uint32_t)ptab->epoch;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t i0 = (uint64_t)blockIdx.x * FL_BLOCK + threadIdx.x;
    const bool live = i0 < n;
    const uint64_t i = live ? i0 : n - 1;
    const uint2 st = *(const uint2*)((const uint32_t*)(rows + 3 * i) + 10);   // {slot, TCP flags}
    const bool keyed = live && st.x != ZP_FLOW_NONE;
    uint32_t f = ZP_FLOW_NONE;
    if (keyed) f = (st.x & FL_TAG) ? st.x & ~FL_TAG : tab[2 * (uint64_t)st.x];
    const bool valid = f < max_flows;                  // ZP_FLOW_NONE: not keyed, or refused
    if (live && flow_of) flow_of[i] = valid ? f : ZP_FLOW_NONE;
    const uint64_t rb = __ballot(keyed && !valid);
    if (rb && lane == 0) fl_add(&hdr->refused, (uint32_t)__builtin_popcountll(rb));
    const uint32_t len = valid ? lens[i] : 0u, tf = valid ? st.y & 0xFFu : 0u;
    bool done = !valid;
    if (COMBINE) {                                     // as zp_flow_label_kernel
        uint64_t rem = __ballot(!done);
        for (int round = 0; round < 2 && rem; ++round) {
            const int ld = __builtin_ctzll(rem);
            const bool same = !done && f == (uint32_t)__builtin_amdgcn_readlane((int)f, ld);
            const uint64_t g = __ballot(same);
            const uint32_t cnt = (uint32_t)__builtin_popcountll(g);
            if (cnt == 1) break;
            const uint64_t bytes = fl_wave_sum(same ? len : 0u);
            uint32_t fo = same ? tf : 0u;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) fo |= __shfl_xor(fo, o);
            if ((int)lane == ld) fl_state_add(flows, f, epoch, cnt, bytes, fo);
            done = done || same;
            rem &= ~g;
        }
    }
    if (!done) fl_state_add(flows, f, epoch, 1u, len, tf);
}

// ---- finish --------------------------------------------------------------------
// One lane. `empty`: a call with n == 0, whose scratch holds nothing.
__global__ void zp_flow_table_finish_kernel(FlTable* __restrict__ ptab, uint64_t sig,
                                            uint64_t max_flows, const FlHdr* __restrict__ hdr,
                                            int empty, uint64_t* __restrict__ count) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (!fl_table_ok(ptab, sig)) {
        count[7] = 1;
        return;
    }
    uint64_t k = 0, t = 0, r = 0, refused = 0;
    if (!empty) {
        for (int c = 0; c < FL_CNT; ++c) {
            k += hdr->cnt[c][0];
            t += hdr->cnt[c][1];
        }
        r = hdr->flows;
        refused = hdr->refused;
    }
    const uint64_t f0 = fl_min64(ptab->flows, max_flows), e = ptab->epoch;
    const uint64_t admitted = fl_min64(r, max_flows - f0);
    count[0] = f0 + admitted;
    count[1] = admitted;
    count[2] = k;
    count[3] = t;
    count[4] = r - admitted;
    count[5] = refused;
    count[6] = e;
    count[7] = 0;
    ptab->flows = f0 + admitted;
    ptab->epoch = e + 1;
}

// ---- retire --------------------------------------------------------------------
// Six launches; again a launch reads by plain loads only what an earlier one
// wrote: mark reads flows and the header; scan the tile counts; move reads
// flows, ballots and sums and writes the staging copy, `retired` and `remap`;
// back reads the staging copy and F' and writes flows[0, F') and the cleared
// slots; insert reads those keys and claims slots by CAS; finish writes the
// header and `count`.
__global__ void __launch_bounds__(FL_BLOCK)
zp_flow_retire_mark_kernel(const FlTable* __restrict__ ptab, uint64_t sig, uint64_t max_flows,
                           const uint64_t* __restrict__ flows, uint32_t max_idle, uint32_t tcp_any,
                           uint64_t* __restrict__ ballots, uint32_t* __restrict__ part) {
    __shared__ uint32_t ws[FL_WAVES];
    if (!fl_table_ok(ptab, sig)) return;
    const uint64_t F = fl_min64(ptab->flows, max_flows);
    const uint32_t epoch = (uint32_t)ptab->epoch;
    const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const uint64_t f = (uint64_t)blockIdx.x * FL_BLOCK + threadIdx.x;
    bool keep = false;
    if (f < F) {
        const uint64_t* const e = flows + 8 * f;
        const uint32_t last = (uint32_t)(e[5] >> 32), tf = (uint32_t)(e[6] >> 56);
        const bool idle = max_idle != ZP_FLOW_IDLE_NEVER && (uint32_t)(epoch - 1u - last) >= max_idle;
        keep = !idle && !(tf & tcp_any);
    }
    const uint64_t b = __ballot(keep);
    if (lane == 0) {
        if (f < max_flows) ballots[f >> 6] = b;
        ws[wid] = (uint32_t)__builtin_popcountll(b);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t c = 0;
        for (int w = 0; w < FL_WAVES; ++w) c += ws[w];
        part[blockIdx.x] = c;
    }
}

__device__ __forceinline__ void fl_copy_entry(uint64_t* dst, const uint64_t* src) {
    const uint4* const s = (const uint4*)src;
    uint4* const d = (uint4*)dst;
    const uint4 a = s[0], b = s[1], c = s[2], e = s[3];
    d[0] = a;
    d[1] = b;
    d[2] = c;
    d[3] = e;
}

__global__ void __launch_bounds__(FL_BLOCK)
zp_flow_retire_move_kernel(const FlTable* __restrict__ ptab, uint64_t sig, uint64_t max_flows,
                           const uint64_t* __restrict__ flows, const uint64_t* __restrict__ ballots,
                           const uint32_t* __restrict__ part, const uint32_t* __restrict__ tot,
                           uint64_t* __restrict__ stage, uint64_t* __restrict__ retired,
                           uint32_t* __restrict__ remap) {
    __shared__ uint32_t ws[FL_WAVES];
    if (!fl_table_ok(ptab, sig)) return;
    const uint64_t F = fl_min64(ptab->flows, max_flows);
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t tile = blockIdx.x;
    const uint64_t f = tile * FL_BLOCK + threadIdx.x;
    const uint64_t w0 = f - lane;
    const uint64_t b = w0 < max_flows ? ballots[w0 >> 6] : 0;
    const bool keep = (b >> lane) & 1u;
    const uint32_t rank = fl_rank(b, ws, part, tot, tile);   // survivors below f
    if (f >= F) return;
    if (keep) {
        fl_copy_entry(stage + 8 * (uint64_t)rank, flows + 8 * f);
        if (remap) remap[f] = rank;
    } else {
        if (retired) fl_copy_entry(retired + 8 * (f - rank), flows + 8 * f);
        if (remap) remap[f] = ZP_FLOW_NONE;
    }
}

__global__ void __launch_bounds__(FL_BLOCK)
zp_flow_retire_back_kernel(FlTable* __restrict__ ptab, uint64_t sig, uint64_t max_flows, uint64_t slots,
                           const FlRetHdr* __restrict__ hdr, const uint64_t* __restrict__ stage,
                           uint64_t* __restrict__ flows) {
    if (!fl_table_ok(ptab, sig)) return;
    const uint64_t F1 = fl_min64(hdr->flows, max_flows);
    const uint64_t g = (uint64_t)blockIdx.x * FL_BLOCK + threadIdx.x;
    if (g < F1) fl_copy_entry(flows + 8 * g, stage + 8 * g);
    if (g < slots) ((uint32_t*)(ptab + 1))[g] = FL_EMPTY;
}

__global__ void __launch_bounds__(FL_BLOCK)
zp_flow_retire_insert_kernel(FlTable* __restrict__ ptab, uint64_t sig, uint64_t max_flows,
                             uint32_t pmask, uint64_t hash_mask, const FlRetHdr* __restrict__ hdr,
                             const uint64_t* __restrict__ flows) {
    if (!fl_table_ok(ptab, sig)) return;
    const uint64_t F1 = fl_min64(hdr->flows, max_flows);
    const uint64_t f = (uint64_t)blockIdx.x * FL_BLOCK + threadIdx.x;
    if (f >= F1) return;
    const uint4* const o = (const uint4*)(flows + 8 * f);
    const uint4 a = o[0], b = o[1];
    const uint2 e = *(const uint2*)(o + 2);
    const uint32_t kw[10] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, e.x, e.y};
    fl_claim((uint32_t*)(ptab + 1), pmask, fl_hash32(kw, hash_mask), (uint32_t)f);
}

__global__ void zp_flow_retire_finish_kernel(FlTable* __restrict__ ptab, uint64_t sig,
                                             uint64_t max_flows, const FlRetHdr* __restrict__ hdr,
                                             uint64_t* __restrict__ count) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (!fl_table_ok(ptab, sig)) {
        count[1] = ~0ull;
        return;
    }
    const uint64_t F = fl_min64(ptab->flows, max_flows), F1 = fl_min64(hdr->flows, F);
    count[0] = F1;
    count[1] = F - F1;
    ptab->flows = F1;
}

// ---- host (table) ----------------------------------------------------------------
static uint64_t fl_pslots(uint64_t max_flows) {
    if (max_flows > FL_MAX_TABLE_FLOWS) max_flows = FL_MAX_TABLE_FLOWS;
    uint64_t t = 64;
    while (t < 2 * max_flows) t <<= 1;
    return t;
}

extern "C" uint64_t zp_flow_table_bytes(uint64_t max_flows) {
    return sizeof(FlTable) + 4 * fl_pslots(max_flows);
}

extern "C" uint64_t zp_flow_update_scratch_bytes(uint64_t n) {
    if (n >= (1ull << 31)) n = (1ull << 31) - 1;       // refused by the call
    return zp_flow_scratch_bytes(n, n);
}

extern "C" uint64_t zp_flow_retire_scratch_bytes(uint64_t max_flows) {
    if (max_flows > FL_MAX_TABLE_FLOWS) max_flows = FL_MAX_TABLE_FLOWS;
    return 16 + sizeof(FlRetHdr) + 64 * max_flows + fl_up16(8 * ((max_flows + 63) / 64)) +
           fl_up16(4 * fl_tiles(max_flows)) + fl_up16(4 * fl_spans(max_flows));
}

static uint64_t fl_sig(const zp_flow_opts* o) {
    const uint32_t kw[10] = {o->key_flags, 0x7A70666Cu, (uint32_t)o->max_flows, (uint32_t)(o->max_flows >> 32),
                             (uint32_t)o->hash_mask, (uint32_t)(o->hash_mask >> 32), 0, 0, 0, 0};
    return fl_hash(kw);
}

static int fl_refuse(const char* fn, const char* what) {
    snprintf(zp__errbuf(), 256, "%s: %s", fn, what);
    return -1;
}

// The refusals the three table calls share; 0 when there is none.
static int fl_table_args(const char* fn, const zp_flow_opts* opts, const void* table,
                         uint64_t table_bytes) {
    if (!opts) return fl_refuse(fn, "null opts");
    if (opts->key_flags & ~(ZP_FLOW_PORTS | ZP_FLOW_PROTO | ZP_FLOW_VLAN | ZP_FLOW_BIDIR))
        return fl_refuse(fn, "unknown key_flags bits");
    if (opts->pad) return fl_refuse(fn, "pad must be 0");
    if (opts->max_flows == 0) return fl_refuse(fn, "max_flows must not be 0");
    if (opts->max_flows > FL_MAX_TABLE_FLOWS) return fl_refuse(fn, "max_flows above 2^30");
    if (!table) return fl_refuse(fn, "null table");
    if (table_bytes < zp_flow_table_bytes(opts->max_flows))
        return fl_refuse(fn, "table_bytes below zp_flow_table_bytes(max_flows)");
    if ((uintptr_t)table & 7) return fl_refuse(fn, "misaligned pointer");
    return 0;
}

extern "C" int zp_flow_table_init_device(void* table, uint64_t table_bytes, const zp_flow_opts* opts,
                                         void* stream) {
    static const char fn[] = "zp_flow_table_init_device";
    int rc;
    if ((rc = fl_table_args(fn, opts, table, table_bytes))) return rc;
    const uint64_t slots = fl_pslots(opts->max_flows);
    hipLaunchKernelGGL(zp_flow_table_init_kernel, dim3((unsigned)fl_tiles(slots)), dim3(FL_BLOCK), 0,
                       (hipStream_t)stream, (FlTable*)table, fl_sig(opts), slots);
    return fl_launched("zp_flow_table_init_kernel");
}

extern "C" int zp_flow_update_device(const uint8_t* arena, const uint64_t* offs, const uint32_t* lens,
                                     const zp_record* records, uint64_t n, const zp_flow_opts* opts,
                                     const uint64_t* mask, void* table, uint64_t table_bytes,
                                     zp_flow_state* flows, uint32_t* flow_of, uint64_t* count,
                                     void* scratch, uint64_t scratch_bytes, void* stream) {
    static const char fn[] = "zp_flow_update_device";
    int rc;
    if ((rc = fl_table_args(fn, opts, table, table_bytes))) return rc;
    if (!count) return fl_refuse(fn, "null count");
    if (!flows) return fl_refuse(fn, "null flows");
    if (((uintptr_t)count & 7) || ((uintptr_t)flows & 15) || ((uintptr_t)mask & 7) ||
        ((uintptr_t)flow_of & 3))
        return fl_refuse(fn, "misaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    FlTable* const ptab = (FlTable*)table;
    const uint64_t sig = fl_sig(opts), max_flows = opts->max_flows;
    if (n == 0) {
        hipLaunchKernelGGL(zp_flow_table_finish_kernel, dim3(1), dim3(64), 0, st, ptab, sig, max_flows,
                           (const FlHdr*)nullptr, 1, count);
        return fl_launched("zp_flow_table_finish_kernel");
    }
    if (!records) return fl_refuse(fn, "null records");
    if (!lens) return fl_refuse(fn, "null lens");
    if (!arena) return fl_refuse(fn, "null arena");
    if (!offs) return fl_refuse(fn, "null offs");
    if (n >= (1ull << 31)) return fl_refuse(fn, "a row's slot word holds a tag bit: n must be below 2^31");
    if (!scratch || scratch_bytes < zp_flow_update_scratch_bytes(n))
        return fl_refuse(fn, "scratch is null or below zp_flow_update_scratch_bytes(n)");
    const uint64_t tiles = fl_tiles(n), spans = fl_spans(n), slots = fl_slots(n, n);
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
    const uint32_t tmask = (uint32_t)(slots - 1), pmask = (uint32_t)(fl_pslots(max_flows) - 1);
    const dim3 grid((unsigned)tiles), block(FL_BLOCK);
    const FlTable* const ctab = ptab;
    hipLaunchKernelGGL(zp_flow_key_kernel<true>, grid, block, 0, st, arena, offs, lens, records, n, mask,
                       opts->key_flags, opts->hash_mask, rows, (uint64_t*)tab, slots, hdr, ctab, sig);
    if ((rc = fl_launched("zp_flow_key_kernel"))) return rc;
    if (fl_combine)
        hipLaunchKernelGGL(zp_flow_find_kernel<true>, grid, block, 0, st, n, rows, tab, tmask, hdr, ctab,
                           sig, pmask, (const uint64_t*)flows, max_flows);
    else
        hipLaunchKernelGGL(zp_flow_find_kernel<false>, grid, block, 0, st, n, rows, tab, tmask, hdr, ctab,
                           sig, pmask, (const uint64_t*)flows, max_flows);
    if ((rc = fl_launched("zp_flow_find_kernel"))) return rc;
    hipLaunchKernelGGL(zp_flow_mark_kernel<true>, grid, block, 0, st, lens, n, rows, tab, ballots, part,
                       hdr, ctab, sig);
    if ((rc = fl_launched("zp_flow_mark_kernel"))) return rc;
    if (spans == 1) {
        hipLaunchKernelGGL(zp_flow_scan_kernel<true>, dim3(1), block, 0, st, part, tiles,
                           (uint32_t*)nullptr, &hdr->flows, 0, ctab, sig);
    } else {
        hipLaunchKernelGGL(zp_flow_scan_kernel<true>, dim3((unsigned)spans), block, 0, st, part, tiles,
                           tot, (uint64_t*)nullptr, 0, ctab, sig);
        if ((rc = fl_launched("zp_flow_scan_kernel"))) return rc;
        hipLaunchKernelGGL(zp_flow_scan_kernel<true>, dim3(1), block, 0, st, tot, spans,
                           (uint32_t*)nullptr, &hdr->flows, 1, ctab, sig);
    }
    if ((rc = fl_launched("zp_flow_scan_kernel"))) return rc;
    hipLaunchKernelGGL(zp_flow_admit_kernel, grid, block, 0, st, n, rows, tab, ballots, part,
                       spans == 1 ? (const uint32_t*)nullptr : tot, max_flows, opts->hash_mask,
                       (uint64_t*)flows, ptab, sig, pmask);
    if ((rc = fl_launched("zp_flow_admit_kernel"))) return rc;
    if (fl_combine)
        hipLaunchKernelGGL(zp_flow_table_label_kernel<true>, grid, block, 0, st, lens, n, rows, tab,
                           flow_of, (uint64_t*)flows, hdr, ctab, sig, max_flows);
    else
        hipLaunchKernelGGL(zp_flow_table_label_kernel<false>, grid, block, 0, st, lens, n, rows, tab,
                           flow_of, (uint64_t*)flows, hdr, ctab, sig, max_flows);
    if ((rc = fl_launched("zp_flow_table_label_kernel"))) return rc;
    hipLaunchKernelGGL(zp_flow_table_finish_kernel, dim3(1), dim3(64), 0, st, ptab, sig, max_flows,
                       (const FlHdr*)hdr, 0, count);
    return fl_launched("zp_flow_table_finish_kernel");
}

extern "C" int zp_flow_retire_device(const zp_flow_opts* opts, void* table, uint64_t table_bytes,
                                     zp_flow_state* flows, uint32_t max_idle, uint32_t tcp_any,
                                     zp_flow_state* retired, uint32_t* remap, uint64_t* count,
                                     void* scratch, uint64_t scratch_bytes, void* stream) {
    static const char fn[] = "zp_flow_retire_device";
    int rc;
    if ((rc = fl_table_args(fn, opts, table, table_bytes))) return rc;
    if (!count) return fl_refuse(fn, "null count");
    if (!flows) return fl_refuse(fn, "null flows");
    if (tcp_any > 0xFFu) return fl_refuse(fn, "tcp_any above 0xFF");
    if (!scratch || scratch_bytes < zp_flow_retire_scratch_bytes(opts->max_flows))
        return fl_refuse(fn, "scratch is null or below zp_flow_retire_scratch_bytes(max_flows)");
    if (((uintptr_t)count & 7) || ((uintptr_t)flows & 15) || ((uintptr_t)retired & 15) ||
        ((uintptr_t)remap & 3))
        return fl_refuse(fn, "misaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    FlTable* const ptab = (FlTable*)table;
    const FlTable* const ctab = ptab;
    const uint64_t sig = fl_sig(opts), m = opts->max_flows, slots = fl_pslots(m);
    const uint64_t tiles = fl_tiles(m), spans = fl_spans(m);
    uint8_t* p = (uint8_t*)(((uintptr_t)scratch + 15) & ~(uintptr_t)15);
    FlRetHdr* const hdr = (FlRetHdr*)p;
    p += sizeof(FlRetHdr);
    uint64_t* const stage = (uint64_t*)p;
    p += 64 * m;
    uint64_t* const ballots = (uint64_t*)p;
    p += fl_up16(8 * ((m + 63) / 64));
    uint32_t* const part = (uint32_t*)p;
    p += fl_up16(4 * tiles);
    uint32_t* const tot = (uint32_t*)p;
    const dim3 grid((unsigned)tiles), block(FL_BLOCK);
    hipLaunchKernelGGL(zp_flow_retire_mark_kernel, grid, block, 0, st, ctab, sig, m,
                       (const uint64_t*)flows, max_idle, tcp_any, ballots, part);
    if ((rc = fl_launched("zp_flow_retire_mark_kernel"))) return rc;
    if (spans == 1) {
        hipLaunchKernelGGL(zp_flow_scan_kernel<true>, dim3(1), block, 0, st, part, tiles,
                           (uint32_t*)nullptr, &hdr->flows, 0, ctab, sig);
    } else {
        hipLaunchKernelGGL(zp_flow_scan_kernel<true>, dim3((unsigned)spans), block, 0, st, part, tiles,
                           tot, (uint64_t*)nullptr, 0, ctab, sig);
        if ((rc = fl_launched("zp_flow_scan_kernel"))) return rc;
        hipLaunchKernelGGL(zp_flow_scan_kernel<true>, dim3(1), block, 0, st, tot, spans,
                           (uint32_t*)nullptr, &hdr->flows, 1, ctab, sig);
    }
    if ((rc = fl_launched("zp_flow_scan_kernel"))) return rc;
    hipLaunchKernelGGL(zp_flow_retire_move_kernel, grid, block, 0, st, ctab, sig, m,
                       (const uint64_t*)flows, (const uint64_t*)ballots, (const uint32_t*)part,
                       spans == 1 ? (const uint32_t*)nullptr : (const uint32_t*)tot, stage,
                       (uint64_t*)retired, remap);
    if ((rc = fl_launched("zp_flow_retire_move_kernel"))) return rc;
    hipLaunchKernelGGL(zp_flow_retire_back_kernel, dim3((unsigned)fl_tiles(slots)), block, 0, st, ptab, sig,
                       m, slots, (const FlRetHdr*)hdr, (const uint64_t*)stage, (uint64_t*)flows);
    if ((rc = fl_launched("zp_flow_retire_back_kernel"))) return rc;
    hipLaunchKernelGGL(zp_flow_retire_insert_kernel, grid, block, 0, st, ptab, sig, m,
                       (uint32_t)(slots - 1), opts->hash_mask, (const FlRetHdr*)hdr,
                       (const uint64_t*)flows);
    if ((rc = fl_launched("zp_flow_retire_insert_kernel"))) return rc;
    hipLaunchKernelGGL(zp_flow_retire_finish_kernel, dim3(1), dim3(64), 0, st, ptab, sig, m,
                       (const FlRetHdr*)hdr, count);
    return fl_launched("zp_flow_retire_finish_kernel");
}
