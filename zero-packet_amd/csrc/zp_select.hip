// zp_select.hip — select and gather: choose parsed frames on the device and
// hand them on as a sub-batch (include/zero_packet.h, zp_select_device,
// zp_gather_frames_device).
//
// Select is three launches on the caller's stream; no kernel waits on another
// workgroup, the stream orders the phases:
//   mark     one lane per frame evaluates the selector; a wave's verdicts leave
//            as one 64-bit ballot word, a 256-frame tile leaves {selected,
//            selected bytes} in scratch. Without terms the frames are not
//            read: the 8-B records (and lens) are streamed as zp_stats_kernel
//            streams them. With terms the header window is staged as in
//            zp_columns_kernel (zp_win.h), the record decoded by the same
//            routines (zp_colrec.h) and the terms evaluated from registers on
//            the values col_values() (zp_cols.h) hands out: no column is stored.
//   scan     exclusive sums of the tiles' pairs, SL_SPAN tiles per workgroup,
//            and a second launch over the workgroups' totals when there is
//            more than one; the totals go to `count`.
//   scatter  from the ballot words and the scanned bases: rank by mbcnt, an
//            in-wave scan of the selected lens, stores of idx / packed_offs.
//
// Gather: element gathers of the descriptors, records and ext entries, and
// the frame copy, organised by destination (see zp_gather_kernel).

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/zero_packet.h"
#include "zp_colrec.h"

extern "C" char* zp__errbuf(void);
extern "C" int zp_col_width(int col);

#define SL_BLOCK FX_BLOCK          // frames per tile: one {count, bytes} pair in scratch
#define SL_WAVES (SL_BLOCK / 64)
#define SL_U 8                     // record-only mark: tiles per workgroup, one load per tile in
                                   // flight per lane (4 KiB of records per wave)
#define SL_PER 4                   // scan: tiles per lane
#define SL_SPAN (SL_BLOCK * SL_PER)   // scan: tiles per workgroup

static_assert(ZP_SELECT_SCAN_FRAMES == (uint64_t)SL_SPAN * SL_BLOCK, "zero_packet.h states the span");
static_assert(sizeof(zp_select_term) == 40, "zp_select_term is 40 bytes");

// The selector as the kernels take it (a kernel argument, built on the host
// from zp_select): term operands as dwords, cut to the column's width.
struct SelTerm {
    uint32_t col, op;
    uint32_t a[4], b[4];
};
struct SelArgs {
    uint32_t all, any, none;
    int32_t err;
    uint32_t min_len, max_len;
    uint32_t nterms;
    uint32_t colmask;              // bit c: a term names column c
    SelTerm t[ZP_SELECT_MAX_TERMS];
};

// Column groups by the header their getters read (col_values' l3 / inner / l4).
#define SL_COLS_L3    (((1u << (ZP_COL_IP_LEN + 1)) - 1u) & ~((1u << ZP_COL_ARP_OPER) - 1u))
#define SL_COLS_INNER (((1u << (ZP_COL_INNER_PROTOCOL + 1)) - 1u) & ~((1u << ZP_COL_INNER_VERSION) - 1u))
#define SL_COLS_L4    (((1u << ZP_COL_COUNT) - 1u) & ~((1u << ZP_COL_L4_PROTO) - 1u))

__device__ __forceinline__ bool sl_term(const SelTerm& t, const uint4 v) {
    const bool m = t.op >= ZP_SEL_RANGE
        ? v.x >= t.a[0] && v.x <= t.b[0]
        : (v.x & t.b[0]) == t.a[0] && (v.y & t.b[1]) == t.a[1] && (v.z & t.b[2]) == t.a[2] &&
          (v.w & t.b[3]) == t.a[3];
    return m != (bool)(t.op & 1u);           // MASK_NE, NOT_RANGE: the odd codes
}

// The record predicate: flags, err (the record's first word) and the length.
__device__ __forceinline__ bool sl_record(const SelArgs& a, uint32_t w0, uint32_t len) {
    const uint32_t f = w0 & ZP_F_MASK, e = w0 >> 26;
    bool p = (f & a.all) == a.all && (f & a.none) == 0 && (a.any == 0 || (f & a.any) != 0);
    p = p && (a.err == ZP_SEL_ERR_ANY || (a.err == ZP_SEL_ERR_NONZERO ? e != 0 : e == (uint32_t)a.err));
    return p && len >= a.min_len && len <= a.max_len;
}

// col_values' sink that evaluates the terms: bit k of `pass` says whether
// term k holds. It starts from the all-zero value of every column (an absent
// reader, an error record) and each value handed in replaces the verdicts of
// the terms on its column.
struct SelSink {
    const SelArgs& a;
    uint32_t pass;
    static constexpr bool kStore = false;
    __device__ __forceinline__ bool l3() const { return (a.colmask & SL_COLS_L3) != 0; }
    __device__ __forceinline__ bool inner() const { return (a.colmask & SL_COLS_INNER) != 0; }
    __device__ __forceinline__ bool l4() const { return (a.colmask & SL_COLS_L4) != 0; }
    __device__ __forceinline__ bool wants(int col) const { return (a.colmask >> col) & 1u; }
    __device__ __forceinline__ void value(int col, const uint4 v) {
#pragma unroll
        for (int k = 0; k < ZP_SELECT_MAX_TERMS; ++k)
            if (k < (int)a.nterms && a.t[k].col == (uint32_t)col)     // wave-uniform
                pass = sl_term(a.t[k], v) ? pass | (1u << k) : pass & ~(1u << k);
    }
    __device__ __forceinline__ void init() {
        pass = 0;
#pragma unroll
        for (int k = 0; k < ZP_SELECT_MAX_TERMS; ++k)
            if (k < (int)a.nterms && sl_term(a.t[k], make_uint4(0, 0, 0, 0))) pass |= 1u << k;
    }
    template <class R>
    __device__ __forceinline__ void mac(int col, R& rd, uint32_t x) {        // as col_mac
        if (!wants(col)) return;
        uint4 v = make_uint4(0, 0, 0, 0);
        v.x = rd_le(rd, x, 2);
        v.x |= rd_le(rd, x + 2, 2) << 16;
        v.y = rd_le(rd, x + 4, 2);
        value(col, v);
    }
    template <class R>
    __device__ __forceinline__ void addr(int col, R& rd, uint32_t x, bool v6) {   // as col_addr
        if (!wants(col)) return;
        uint4 v;
        v.x = rd_le(rd, x, 4);
        v.y = v6 ? rd_le(rd, x + 4, 4) : 0u;
        v.z = v6 ? rd_le(rd, x + 8, 4) : 0u;
        v.w = v6 ? rd_le(rd, x + 12, 4) : 0u;
        value(col, v);
    }
    template <typename T>
    __device__ __forceinline__ void put(int col, T v) {
        if (wants(col)) value(col, make_uint4((uint32_t)v, 0, 0, 0));
    }
};

// Sum of a u32 over the wave, exact in 64 bits (two 16-bit halves, each sum
// below 2^22).
__device__ __forceinline__ uint64_t sl_wave_sum(uint32_t v) {
    uint32_t lo = v & 0xFFFFu, hi = v >> 16;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo += __shfl_xor(lo, o);
        hi += __shfl_xor(hi, o);
    }
    return ((uint64_t)hi << 16) + lo;
}

// ---- mark, record-only -----------------------------------------------------
// A workgroup takes SL_U consecutive tiles; lane t of it loads record
// t + 256 u of each (coalesced 512-B wave loads, SL_U in flight), and lens[]
// the same way when there is one.
__global__ void __launch_bounds__(SL_BLOCK)
zp_select_mark_rec_kernel(const uint32_t* __restrict__ lens, const zp_record* __restrict__ recs,
                          uint64_t n, uint64_t ntiles, SelArgs a, uint64_t* __restrict__ ballots,
                          uint64_t* __restrict__ part) {
    __shared__ uint64_t ws[SL_U][SL_WAVES][2];
    const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const uint64_t base = (uint64_t)blockIdx.x * (SL_U * SL_BLOCK) + threadIdx.x;
    zp_u32x2 q[SL_U];
    uint32_t l[SL_U];
#pragma unroll
    for (int u = 0; u < SL_U; ++u) {
        const uint64_t i = base + (uint64_t)u * SL_BLOCK;
        const uint64_t ic = i < n ? i : n - 1;
        q[u] = __builtin_nontemporal_load((const FX_GLOBAL zp_u32x2*)(recs + ic));
        l[u] = lens ? lens[ic] : 0u;
    }
#pragma unroll
    for (int u = 0; u < SL_U; ++u) {
        const uint64_t i = base + (uint64_t)u * SL_BLOCK;
        // without lens there is no length bound (refused on the host): 0 passes
        const bool sel = i < n && sl_record(a, q[u].x, lens ? l[u] : a.min_len);
        const uint64_t b = __ballot(sel);
        const uint64_t bytes = sl_wave_sum(sel ? l[u] : 0u);
        if (lane == 0) {
            if (i < n) ballots[i >> 6] = b;           // i: the wave's first frame
            ws[u][wid][0] = (uint64_t)__builtin_popcountll(b);
            ws[u][wid][1] = bytes;
        }
    }
    __syncthreads();
    if (threadIdx.x < SL_U) {
        const uint64_t tile = (uint64_t)blockIdx.x * SL_U + threadIdx.x;
        if (tile < ntiles) {
            uint64_t c = 0, s = 0;
            for (int w = 0; w < SL_WAVES; ++w) {
                c += ws[threadIdx.x][w][0];
                s += ws[threadIdx.x][w][1];
            }
            part[2 * tile] = c;
            part[2 * tile + 1] = s;
        }
    }
}

// ---- mark, with terms ------------------------------------------------------
// One tile per workgroup, one lane per frame, the header window staged and
// the record decoded as in zp_columns_kernel. A frame the record predicate
// already leaves out is not staged.
__global__ void __launch_bounds__(SL_BLOCK)
zp_select_mark_terms_kernel(const uint8_t* __restrict__ arena, const uint64_t* __restrict__ offs,
                            const uint32_t* __restrict__ lens, const zp_record* __restrict__ recs,
                            uint64_t n, SelArgs a, uint64_t* __restrict__ ballots,
                            uint64_t* __restrict__ part) {
    __shared__ uint4 win[FX_CH * FX_BLOCK];
    __shared__ uint64_t ws[SL_WAVES][2];
    const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const uint64_t i0 = (uint64_t)blockIdx.x * FX_BLOCK + threadIdx.x;
    // Lanes past the batch stay for the cooperative staging and the ballot.
    const bool live = i0 < n;
    const uint64_t i = live ? i0 : n - 1;
    zp_rec_full r;
    const zp_u32x2 q = *(const FX_GLOBAL zp_u32x2*)(recs + i);
    const bool far = fx_rec_decode(q, r);            // zp_colrec.h
    const uint32_t ln = lens[i];
    const bool pre = live && sl_record(a, q.x, ln);
    const bool ok = pre && r.err == 0 && (r.flags & ZP_F_ETHERNET);
    const uint32_t len = ok ? ln : 0u;
    const uintptr_t ga = (uintptr_t)arena + (ok ? offs[i] : 0);
    SelSink s{a, 0u};
    s.init();
    Hdr h;
    h.g = (const uint8_t*)ga;
    h.shift = (uint32_t)(ga & 15);
    // Stage only as far as the terms' columns read.
    uint32_t need = fx_rec_need(r, ok, far, s.l3(), s.inner(), s.l4());
    need = need < len ? need : len;
    h.wlen = need < FX_WIN - h.shift ? need : FX_WIN - h.shift;
    h.win = (const uint8_t*)&win[threadIdx.x];
    h.xc = make_uint4(0, 0, 0, 0);
    h.xi = ~0u;
    fx_stage(win, ga, len, h);

    HdrReader rd{h};
    // the far form's eth_len is read by every getter; the final next headers
    // only by the outer / inner IP groups
    fx_rec_finish(rd, r, ok && (far || s.l3() || s.inner()), far);
    col_values(rd, r, ok, len, s);
    const bool sel = pre && s.pass == (1u << a.nterms) - 1u;
    const uint64_t b = __ballot(sel);
    const uint64_t bytes = sl_wave_sum(sel ? ln : 0u);
    if (lane == 0) {
        if (live) ballots[i0 >> 6] = b;
        ws[wid][0] = (uint64_t)__builtin_popcountll(b);
        ws[wid][1] = bytes;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t c = 0, t = 0;
        for (int w = 0; w < SL_WAVES; ++w) {
            c += ws[w][0];
            t += ws[w][1];
        }
        part[2 * (uint64_t)blockIdx.x] = c;
        part[2 * (uint64_t)blockIdx.x + 1] = t;
    }
}

// ---- scan ------------------------------------------------------------------
// Exclusive sums over `m` {count, bytes} pairs, in place. A workgroup covers
// SL_SPAN pairs; `loop`: one workgroup walks the whole array span by span
// with a carry (the second level). Totals: to tot[2 b] of workgroup b, and to
// `count` when this launch sees the whole array.
__global__ void __launch_bounds__(SL_BLOCK)
zp_select_scan_kernel(uint64_t* __restrict__ part, uint64_t m, uint64_t* __restrict__ tot,
                      uint64_t* __restrict__ count, int loop) {
    __shared__ uint64_t ws[SL_WAVES][2];
    const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    uint64_t carry_c = 0, carry_s = 0;
    uint64_t first = loop ? 0 : (uint64_t)blockIdx.x * SL_SPAN;
    const uint64_t last = loop ? m : (first + SL_SPAN < m ? first + SL_SPAN : m);
    for (; first < last; first += SL_SPAN) {
        const uint64_t j0 = first + (uint64_t)threadIdx.x * SL_PER;
        uint64_t c[SL_PER], s[SL_PER], tc = 0, ts = 0;
#pragma unroll
        for (int k = 0; k < SL_PER; ++k) {
            c[k] = j0 + k < last ? part[2 * (j0 + k)] : 0;
            s[k] = j0 + k < last ? part[2 * (j0 + k) + 1] : 0;
            tc += c[k];
            ts += s[k];
        }
        uint64_t ic = tc, is = ts;                    // inclusive over the wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint64_t uc = __shfl_up(ic, o), us = __shfl_up(is, o);
            if (lane >= (uint32_t)o) {
                ic += uc;
                is += us;
            }
        }
        if (lane == 63) {
            ws[wid][0] = ic;
            ws[wid][1] = is;
        }
        __syncthreads();
        uint64_t bc = carry_c, bs = carry_s, allc = 0, alls = 0;
        for (int w = 0; w < SL_WAVES; ++w) {
            if (w < (int)wid) {
                bc += ws[w][0];
                bs += ws[w][1];
            }
            allc += ws[w][0];
            alls += ws[w][1];
        }
        __syncthreads();                              // ws is reused by the next span
        bc += ic - tc;
        bs += is - ts;
#pragma unroll
        for (int k = 0; k < SL_PER; ++k) {
            if (j0 + k < last) {
                part[2 * (j0 + k)] = bc;
                part[2 * (j0 + k) + 1] = bs;
            }
            bc += c[k];
            bs += s[k];
        }
        carry_c += allc;
        carry_s += alls;
    }
    if (threadIdx.x == 0) {
        if (tot) {
            tot[2 * (uint64_t)blockIdx.x] = carry_c;
            tot[2 * (uint64_t)blockIdx.x + 1] = carry_s;
        }
        if (count) {
            count[0] = carry_c;
            count[1] = carry_s;
        }
    }
}

// ---- scatter ---------------------------------------------------------------
template <bool BYTES>
__global__ void __launch_bounds__(SL_BLOCK)
zp_select_scatter_kernel(const uint32_t* __restrict__ lens, uint64_t n,
                         const uint64_t* __restrict__ ballots, const uint64_t* __restrict__ part,
                         const uint64_t* __restrict__ tot, uint32_t* __restrict__ idx,
                         uint64_t* __restrict__ packed) {
    __shared__ uint64_t ws[SL_WAVES][2];
    const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const uint64_t tile = blockIdx.x;
    const uint64_t i = tile * SL_BLOCK + threadIdx.x;
    const uint64_t w0 = i - lane;                      // the wave's first frame
    const uint64_t b = w0 < n ? ballots[w0 >> 6] : 0;  // wave-uniform
    const bool sel = (b >> lane) & 1u;                 // bits at and past n are 0
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32),
                                                    __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
    uint64_t inc = 0, mine = 0;
    if (BYTES) {
        mine = sel ? lens[i] : 0u;
        inc = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint64_t u = __shfl_up(inc, o);
            if (lane >= (uint32_t)o) inc += u;
        }
    }
    if (lane == 63) {
        ws[wid][0] = (uint64_t)__builtin_popcountll(b);
        ws[wid][1] = inc;
    }
    __syncthreads();
    uint64_t bc = part[2 * tile], bs = part[2 * tile + 1];
    if (tot) {
        bc += tot[2 * (tile / SL_SPAN)];
        bs += tot[2 * (tile / SL_SPAN) + 1];
    }
    for (int w = 0; w < (int)wid; ++w) {
        bc += ws[w][0];
        bs += ws[w][1];
    }
    if (sel) {
        if (idx) idx[bc + rank] = (uint32_t)i;
        if (BYTES) packed[bc + rank] = bs + inc - mine;
    }
}

// ---- gather ----------------------------------------------------------------
// A workgroup takes FRAMES consecutive entries of idx (64 or 256, below); a
// lane gathers the descriptor, record and ext entries of one entry. The copy
// is organised by destination: the workgroup's frames lie back to back in
// dst, so its span of dst is cut into the 16-B chunks of dst itself and every
// lane of the four waves takes one chunk per trip, 256 consecutive chunks per
// trip whatever the frame lengths (sixty-four 64-B frames, or less than half
// of a 9,000-B one). This is zp_stream.h's lane -> (frame, chunk) mapping
// turned round: there the chunks are the source's and the frame is found from
// the tile's running lengths, here they are the destination's and the lane
// finds its frame by a search over the workgroup's packed offsets in LDS.
// The builder's wave copy (all 64 lanes on one frame) would leave 60 lanes
// idle on a 64-B frame.
// A chunk wholly inside one frame is one aligned 16-B store; the source bytes
// come from the one or two aligned 16-B chunks that hold them and are
// realigned in registers (v_alignbyte). A chunk at a frame's edge takes, from
// every frame that has bytes in it, exactly those bytes, with dword stores
// where a whole dword is the frame's and byte stores otherwise: nothing
// outside the frames' bytes is written, and no source chunk is read that
// holds none of the frame's bytes.
#define GA_BLOCK 256
#define GA_SHORT 128       // average frame bytes up to which a workgroup takes 256 entries

// FRAMES entries of idx per workgroup: 64 (the first wave gathers them, all
// four waves copy: long frames, where a span of 64 frames is many trips) or
// 256 (every lane gathers one: short frames, where the descriptor gathers are
// a large share of the work). The host picks by the average frame length.
template <int FRAMES>
struct GaLds {
    uint64_t off[FRAMES];      // packed offset of the workgroup's entries (~0: none)
    uint64_t src[FRAMES];      // source address
    uint32_t len[FRAMES];
    uint64_t span[GA_BLOCK / 64][2];
};

__device__ __forceinline__ uint32_t ga_sel(bool c, uint32_t a, uint32_t b) { return c ? a : b; }

template <int FRAMES>
__global__ void __launch_bounds__(GA_BLOCK)
zp_gather_kernel(const uint8_t* __restrict__ arena, const uint64_t* __restrict__ offs,
                 const uint32_t* __restrict__ lens, const zp_record* __restrict__ recs,
                 const zp_ext_offsets* __restrict__ ext, uint64_t n,
                 const uint32_t* __restrict__ idx, const uint64_t* __restrict__ packed, uint64_t m,
                 const uint64_t* __restrict__ count, uint8_t* __restrict__ dst, uint64_t dst_bytes,
                 uint64_t* __restrict__ out_offs, uint32_t* __restrict__ out_lens,
                 zp_record* __restrict__ out_recs, zp_ext_offsets* __restrict__ out_ext) {
    static_assert(FRAMES == 64 || FRAMES == GA_BLOCK, "whole waves gather the entries");
    __shared__ GaLds<FRAMES> L;
    const uint32_t t = threadIdx.x;
    uint64_t cnt = m;
    if (count && *count < cnt) cnt = *count;
    const uint64_t j = (uint64_t)blockIdx.x * FRAMES + t;
    const bool live = t < FRAMES && j < cnt;          // FRAMES == 64: the first wave takes the entries
    uint64_t po = ~0ull, sa = 0;
    uint32_t ln = 0;
    if (live) {
        const uint64_t i = idx[j];
        const bool inb = i < n;                        // an index past the batch gathers nothing
        const uint64_t so = inb ? offs[i] : 0;
        const uint32_t l0 = inb && lens ? lens[i] : 0u;
        if (out_lens) out_lens[j] = l0;
        if (out_recs && inb)
            *(FX_GLOBAL zp_u32x2*)(out_recs + j) = *(const FX_GLOBAL zp_u32x2*)(recs + i);
        if (out_ext && inb) {
            ((uint4*)out_ext)[j] = ((const uint4*)ext)[i];
            ((uint4*)out_ext)[m + j] = ((const uint4*)ext)[n + i];
        }
        if (dst) {
            const uint64_t p = packed[j];
            if (out_offs) out_offs[j] = p;
            // a frame that does not fit [0, dst_bytes) is not copied
            if (inb && p <= dst_bytes && l0 <= dst_bytes - p) {
                po = p;
                sa = (uint64_t)(uintptr_t)arena + so;
                ln = l0;
            }
        } else if (out_offs) {
            out_offs[j] = so;
        }
    }
    if (!dst) return;
    if (t < FRAMES) {
        L.off[t] = po;
        L.src[t] = sa;
        L.len[t] = ln;
        // the workgroup's span of dst: [lo, hi)
        uint64_t lo = po, hi = ln ? po + ln : 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const uint64_t a = __shfl_xor(lo, o), b = __shfl_xor(hi, o);
            lo = a < lo ? a : lo;
            hi = b > hi ? b : hi;
        }
        if ((t & 63) == 0) {
            L.span[t >> 6][0] = lo;
            L.span[t >> 6][1] = hi;
        }
    }
    __syncthreads();
    uint64_t lo = L.span[0][0], hi = L.span[0][1];
    for (int w = 1; w < FRAMES / 64; ++w) {
        lo = L.span[w][0] < lo ? L.span[w][0] : lo;
        hi = L.span[w][1] > hi ? L.span[w][1] : hi;
    }
    if (hi == 0) return;                               // nothing to copy (uniform)
    const uint64_t dmis = (uint64_t)(uintptr_t)dst & 15;
    uint8_t* const dbase = dst - dmis;                 // 16-B aligned; chunk k at dbase + 16 k
    const uint64_t k1 = (dmis + hi + 15) >> 4;
    for (uint64_t k = ((dmis + lo) >> 4) + t; k < k1; k += GA_BLOCK) {
        // packed position of the chunk's first byte (negative in the first chunk of dst)
        const int64_t cp = (int64_t)(16 * k) - (int64_t)dmis;
        const int64_t ce = cp + 16;
        // the last entry whose offset is <= cp (entry 0 if there is none)
        uint32_t g = 0;
#pragma unroll
        for (uint32_t step = FRAMES / 2; step > 0; step >>= 1) {
            const uint64_t o = L.off[g + step];
            if (o != ~0ull && (int64_t)o <= cp) g += step;
        }
        for (; g < FRAMES; ++g) {
            const uint64_t o = L.off[g];
            if (o == ~0ull) continue;                  // not copied
            if ((int64_t)o >= ce) break;
            const uint32_t fl = L.len[g];
            // bytes [b0, b1) of the chunk are this frame's
            const int64_t f0 = (int64_t)o - cp, f1 = f0 + fl;
            const uint32_t b0 = f0 > 0 ? (uint32_t)f0 : 0u, b1 = f1 < 16 ? (uint32_t)(f1 > 0 ? f1 : 0) : 16u;
            if (b1 <= b0) continue;
            // source address of chunk byte 0 (not read unless b0 == 0)
            const uint64_t sb = L.src[g] - (uint64_t)f0;
            const uint64_t a0 = (sb + b0) & ~15ull, a1 = (sb + b1 - 1) & ~15ull;
            const uint4 x0 = fx_ld16((uintptr_t)a0);
            const uint4 x1 = a1 != a0 ? fx_ld16((uintptr_t)a1) : x0;
            // chunk byte b is byte b + t of Y = {16 B unused, x0, x1}, t in [1, 31]
            const uint32_t t = (uint32_t)(sb - a0) + 16u, td = t >> 2, tb = t & 3u;
            uint32_t y[12] = {0, 0, 0, 0, x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
            uint32_t y4[8], y2[6], y1[5];
#pragma unroll
            for (int q = 0; q < 8; ++q) y4[q] = ga_sel(td & 4u, y[q + 4], y[q]);
#pragma unroll
            for (int q = 0; q < 6; ++q) y2[q] = ga_sel(td & 2u, y4[q + 2], y4[q]);
#pragma unroll
            for (int q = 0; q < 5; ++q) y1[q] = ga_sel(td & 1u, y2[q + 1], y2[q]);
            uint32_t v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = __builtin_amdgcn_alignbyte(y1[q + 1], y1[q], tb);
            uint8_t* const d = dbase + 16 * k;
            if (b0 == 0 && b1 == 16) {
                *(FX_GLOBAL fx_u32x4*)d = fx_u32x4{v[0], v[1], v[2], v[3]};
            } else {
#pragma unroll
                for (uint32_t q = 0; q < 4; ++q) {
                    if (b0 <= 4 * q && 4 * q + 4 <= b1) {
                        *(FX_GLOBAL uint32_t*)(d + 4 * q) = v[q];
                    } else {
#pragma unroll
                        for (uint32_t e = 0; e < 4; ++e)
                            if (b0 <= 4 * q + e && 4 * q + e < b1)
                                *(FX_GLOBAL uint8_t*)(d + 4 * q + e) = (uint8_t)(v[q] >> (8 * e));
                    }
                }
            }
        }
    }
}

// ---- host ------------------------------------------------------------------
static uint64_t sl_tiles(uint64_t n) { return (n + SL_BLOCK - 1) / SL_BLOCK; }
static uint64_t sl_spans(uint64_t n) { return (sl_tiles(n) + SL_SPAN - 1) / SL_SPAN; }

// scratch: ceil(n / 64) ballot words, a pair per tile, a pair per scan span
extern "C" uint64_t zp_select_scratch_bytes(uint64_t n) {
    const uint64_t words = (n + 63) / 64 + 2 * sl_tiles(n) + 2 * sl_spans(n);
    return 8 * words + 16;
}

static int sl_fail(const char* what) {
    snprintf(zp__errbuf(), 256, "zp_select_device: %s", what);
    return -1;
}

static int sl_launched(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return 0;
    snprintf(zp__errbuf(), 256, "%s launch: %s", what, hipGetErrorString(e));
    return -2;
}

extern "C" int zp_select_device(const uint8_t* arena, const uint64_t* offs, const uint32_t* lens,
                                const zp_record* records, uint64_t n, const zp_select* sel,
                                uint64_t* mask, uint32_t* idx, uint64_t* packed_offs,
                                uint64_t* count, void* scratch, uint64_t scratch_bytes,
                                void* stream) {
    if (!sel) return sl_fail("null selector");
    if (!count) return sl_fail("null count");
    if (sel->nterms > ZP_SELECT_MAX_TERMS) return sl_fail("more than ZP_SELECT_MAX_TERMS terms");
    SelArgs a;
    memset(&a, 0, sizeof a);
    a.all = sel->flags_all;
    a.any = sel->flags_any;
    a.none = sel->flags_none;
    a.err = sel->err;
    a.min_len = sel->min_len;
    a.max_len = sel->max_len;
    a.nterms = sel->nterms;
    for (uint32_t k = 0; k < sel->nterms; ++k) {
        const zp_select_term& t = sel->terms[k];
        const int w = zp_col_width(t.col);
        if (t.col >= ZP_COL_COUNT || w == 0) {
            snprintf(zp__errbuf(), 256, "zp_select_device: term %u: column %u out of range", k, t.col);
            return -1;
        }
        if (t.op > ZP_SEL_NOT_RANGE) {
            snprintf(zp__errbuf(), 256, "zp_select_device: term %u: unknown op %u", k, t.op);
            return -1;
        }
        for (int p = 0; p < 6; ++p)
            if (t.pad[p]) {
                snprintf(zp__errbuf(), 256, "zp_select_device: term %u: pad must be 0", k);
                return -1;
            }
        if (t.op >= ZP_SEL_RANGE && w > 4) {
            snprintf(zp__errbuf(), 256, "zp_select_device: term %u: RANGE on byte-array column %u",
                     k, t.col);
            return -1;
        }
        uint8_t ab[2][16];
        memset(ab, 0, sizeof ab);
        memcpy(ab[0], t.a, (size_t)w);                 // the column's width, zeros behind
        memcpy(ab[1], t.b, (size_t)w);
        a.t[k].col = t.col;
        a.t[k].op = t.op;
        memcpy(a.t[k].a, ab[0], 16);
        memcpy(a.t[k].b, ab[1], 16);
        a.colmask |= 1u << t.col;
    }
    const bool bounded = sel->min_len != 0 || sel->max_len != UINT32_MAX;
    if (n == 0) {
        if (hipMemsetAsync(count, 0, 16, (hipStream_t)stream) != hipSuccess) {
            snprintf(zp__errbuf(), 256, "zp_select_device: clearing count failed");
            return -2;
        }
        return 0;
    }
    if (!records) return sl_fail("null records");
    if (a.nterms && (!arena || !offs || !lens))
        return sl_fail("terms need arena, offs and lens");
    if (!lens && (packed_offs || bounded))
        return sl_fail("packed_offs and length bounds need lens");
    if (idx && n >= (1ull << 32)) return sl_fail("idx holds 32-bit indices: n must be below 2^32");
    if (!scratch || scratch_bytes < zp_select_scratch_bytes(n))
        return sl_fail("scratch is null or below zp_select_scratch_bytes(n)");
    if (((uintptr_t)mask & 7) || ((uintptr_t)count & 7) || ((uintptr_t)packed_offs & 7) ||
        ((uintptr_t)idx & 3))
        return sl_fail("misaligned output pointer");
    const uint64_t tiles = sl_tiles(n), spans = sl_spans(n);
    if (tiles > 0x7FFFFFFFull) return sl_fail("batch too large");
    uint64_t* const s0 = (uint64_t*)(((uintptr_t)scratch + 15) & ~(uintptr_t)15);
    uint64_t* const ballots = mask ? mask : s0;
    uint64_t* const part = s0 + (n + 63) / 64;
    uint64_t* const tot = part + 2 * tiles;
    hipStream_t st = (hipStream_t)stream;
    int rc;
    if (a.nterms == 0) {
        const uint64_t blocks = (tiles + SL_U - 1) / SL_U;
        hipLaunchKernelGGL(zp_select_mark_rec_kernel, dim3((unsigned)blocks), dim3(SL_BLOCK), 0, st,
                           lens, records, n, tiles, a, ballots, part);
        if ((rc = sl_launched("zp_select_mark_rec_kernel"))) return rc;
    } else {
        hipLaunchKernelGGL(zp_select_mark_terms_kernel, dim3((unsigned)tiles), dim3(SL_BLOCK), 0, st,
                           arena, offs, lens, records, n, a, ballots, part);
        if ((rc = sl_launched("zp_select_mark_terms_kernel"))) return rc;
    }
    if (spans == 1) {
        hipLaunchKernelGGL(zp_select_scan_kernel, dim3(1), dim3(SL_BLOCK), 0, st, part, tiles,
                           (uint64_t*)nullptr, count, 0);
    } else {
        hipLaunchKernelGGL(zp_select_scan_kernel, dim3((unsigned)spans), dim3(SL_BLOCK), 0, st, part,
                           tiles, tot, (uint64_t*)nullptr, 0);
        if ((rc = sl_launched("zp_select_scan_kernel"))) return rc;
        hipLaunchKernelGGL(zp_select_scan_kernel, dim3(1), dim3(SL_BLOCK), 0, st, tot, spans,
                           (uint64_t*)nullptr, count, 1);
    }
    if ((rc = sl_launched("zp_select_scan_kernel"))) return rc;
    if (idx || packed_offs) {
        const uint64_t* const t2 = spans == 1 ? nullptr : tot;
        if (packed_offs)
            hipLaunchKernelGGL(zp_select_scatter_kernel<true>, dim3((unsigned)tiles), dim3(SL_BLOCK),
                               0, st, lens, n, ballots, part, t2, idx, packed_offs);
        else
            hipLaunchKernelGGL(zp_select_scatter_kernel<false>, dim3((unsigned)tiles),
                               dim3(SL_BLOCK), 0, st, lens, n, ballots, part, t2, idx, packed_offs);
        if ((rc = sl_launched("zp_select_scatter_kernel"))) return rc;
    }
    return 0;
}

extern "C" int zp_gather_frames_device(const uint8_t* arena, const uint64_t* offs,
                                       const uint32_t* lens, const zp_record* records,
                                       const zp_ext_offsets* ext, uint64_t n, const uint32_t* idx,
                                       const uint64_t* packed_offs, uint64_t m,
                                       const uint64_t* count, uint8_t* dst, uint64_t dst_bytes,
                                       uint64_t* out_offs, uint32_t* out_lens,
                                       zp_record* out_records, zp_ext_offsets* out_ext,
                                       void* stream) {
    const char* bad = nullptr;
    if (!idx) bad = "null idx";
    else if (!offs) bad = "null offs";
    else if ((out_lens || dst) && !lens) bad = "out_lens and dst need lens";
    else if (out_records && !records) bad = "out_records needs records";
    else if (out_ext && !ext) bad = "out_ext needs ext";
    else if (dst && (!arena || !packed_offs)) bad = "dst needs arena and packed_offs";
    else if (((uintptr_t)out_ext & 15) || ((uintptr_t)ext & 15) || ((uintptr_t)out_records & 7) ||
             ((uintptr_t)out_offs & 7) || ((uintptr_t)out_lens & 3))
        bad = "misaligned pointer";
    else if ((m + 63) / 64 > 0x7FFFFFFFull) bad = "batch too large";
    if (bad) {
        snprintf(zp__errbuf(), 256, "zp_gather_frames_device: %s", bad);
        return -1;
    }
    if (m == 0 || n == 0) return 0;
    // dst_bytes / m: the average frame the caller sized dst for (a view copies nothing)
    if (!dst || dst_bytes / m <= GA_SHORT)
        hipLaunchKernelGGL(zp_gather_kernel<GA_BLOCK>, dim3((unsigned)((m + GA_BLOCK - 1) / GA_BLOCK)),
                           dim3(GA_BLOCK), 0, (hipStream_t)stream, arena, offs, lens, records, ext,
                           n, idx, packed_offs, m, count, dst, dst_bytes, out_offs, out_lens,
                           out_records, out_ext);
    else
        hipLaunchKernelGGL(zp_gather_kernel<64>, dim3((unsigned)((m + 63) / 64)), dim3(GA_BLOCK), 0,
                           (hipStream_t)stream, arena, offs, lens, records, ext, n, idx,
                           packed_offs, m, count, dst, dst_bytes, out_offs, out_lens, out_records,
                           out_ext);
    return sl_launched("zp_gather_kernel");
}
