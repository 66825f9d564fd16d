// zp_classify.hip — classify: a first-match rule table over parsed frames
// (include/zero_packet.h, zp_classify_compile, zp_classify_device).
//
// A rule is a zp_select. zp_classify_compile turns up to 256 of them into a
// table of dwords the kernel walks with wave-uniform addresses:
//   header   CT_HDR dwords: signature, version, nrules, flags, the union of
//            the terms' columns, the counts of distinct predicates / terms;
//   preds    the distinct record predicates {flags_all, flags_any, flags_none,
//            err, min_len, max_len} of the rules, each with the 256-bit set of
//            the rules that carry it;
//   cols     per column: first distinct term and how many (terms are grouped
//            by column);
//   zero     per column: the set of rules with a term on it that fails on the
//            all-zero value;
//   terms    the distinct terms {op, a, b}, each with the set of the rules
//            that carry it (l4_proto == 6 in forty rules is one entry).
// One launch: one lane per frame, tiles of FX_BLOCK frames. A lane keeps the
// set of rules that can still match ("alive") in W dwords, W = 2, 4, 6 or 8 by
// nrules (a template parameter). Every distinct predicate that fails clears
// its rules; then, for a table with terms, the header window is staged once
// as far as the union of the columns reads (zp_win.h, zp_colrec.h) and
// col_values() (zp_cols.h) hands each wanted column's value to ClsSink, which
// loops over that column's distinct terms (operands through scalar loads) and
// clears the rules of those that fail. A byte-array column col_values() never
// hands in (an absent reader, an error record) counts as all zero: its
// `zero` set is cleared instead. rule_of is the lowest bit left.
// The grid is sized to fill the device once and a workgroup walks several
// tiles. Counters: a wave adds the frames of its two leading rules as one
// reduced pair each to the workgroup's LDS histogram, the rest per lane (LDS
// atomics); after its last tile the workgroup issues one global 64-bit
// atomic add per non-zero entry, so a hot rule costs a few thousand global
// atomics per batch, not one per tile.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/zero_packet.h"
#include "zp_colrec.h"

extern "C" char* zp__errbuf(void);
extern "C" int zp_col_width(int col);

#define CT_MAGIC 0x5443505Au       // "ZPCT"
#define CT_VERSION 1u
#define CT_SETW 8                  // dwords of a rule set (256 bits), whatever nrules
#define CT_HDR 16
#define CT_H_MAGIC 0
#define CT_H_VERSION 1
#define CT_H_NRULES 2
#define CT_H_FLAGS 3               // CT_F_*
#define CT_H_COLMASK 4             // bit c: a term names column c
#define CT_H_NPREDS 5
#define CT_H_NTERMS 6              // distinct terms
#define CT_H_BYTES 7               // zp_classify_table_bytes(nrules)
#define CT_F_TERMS 1u              // some rule has terms: the frames are read
#define CT_F_BOUNDED 2u            // some rule bounds the length: lens is needed
#define CT_PRED 16                 // dwords per distinct predicate: 6 used, 2 zero, the set
#define CT_TERM 20                 // dwords per distinct term: op, 3 zero, a[4], b[4], the set
#define CT_COLS 32                 // column slots (ZP_COL_COUNT <= 32)
#define CT_OFF_PREDS CT_HDR
#define CT_OFF_COLS(nr) (CT_OFF_PREDS + CT_PRED * (nr))
#define CT_OFF_ZERO(nr) (CT_OFF_COLS(nr) + 2 * CT_COLS)
#define CT_OFF_TERMS(nr) (CT_OFF_ZERO(nr) + CT_SETW * CT_COLS)
#define CT_WORDS(nr) (CT_OFF_TERMS(nr) + CT_TERM * ZP_SELECT_MAX_TERMS * (nr))

static_assert(ZP_COL_COUNT <= CT_COLS, "a column mask is one dword");
static_assert(ZP_CLASSIFY_MAX_RULES == 32 * CT_SETW, "a rule set is CT_SETW dwords");
static_assert(sizeof(zp_rule_hits) == 16, "zp_rule_hits is two 64-bit words");

// Column groups by the header their getters read (col_values' l3 / inner / l4).
#define CL_COLS_L3    (((1u << (ZP_COL_IP_LEN + 1)) - 1u) & ~((1u << ZP_COL_ARP_OPER) - 1u))
#define CL_COLS_INNER (((1u << (ZP_COL_INNER_PROTOCOL + 1)) - 1u) & ~((1u << ZP_COL_INNER_VERSION) - 1u))
#define CL_COLS_L4    (((1u << ZP_COL_COUNT) - 1u) & ~((1u << ZP_COL_L4_PROTO) - 1u))
// The byte-array columns: col_values() hands them in only for a present reader.
#define CL_COLS_BYTES ((1u << ZP_COL_DEST_MAC) | (1u << ZP_COL_SRC_MAC) | (1u << ZP_COL_SRC_ADDR) | \
                       (1u << ZP_COL_DEST_ADDR) | (1u << ZP_COL_INNER_SRC_ADDR) |                   \
                       (1u << ZP_COL_INNER_DEST_ADDR))

#define CL_BLOCK FX_BLOCK
#define CL_WAVES (CL_BLOCK / 64)
#define CL_ACCW (CT_SETW + 1)      // dwords of `accept`: nrules + 1 bits

// The table is read-only for the launch and every address into it is
// wave-uniform: the constant address space makes those scalar loads.
typedef const __attribute__((address_space(4))) uint32_t* cl_tab;

struct ClsAccept {
    uint32_t w[CL_ACCW];
};

// Operands leave the table in whole 16-B scalar loads issued up front; the
// verdict is computed without short-circuits (a chain of dependent dword loads
// and branches per term cost several times the compares).
typedef uint32_t cl_u32x4 __attribute__((ext_vector_type(4), aligned(4)));
typedef const __attribute__((address_space(4))) cl_u32x4* cl_tab4;

// One term (t: its CT_TERM dwords) on value v -> whether it FAILS; WIDE: a
// byte-array column (the four dwords count).
template <bool WIDE>
__device__ __forceinline__ bool cl_term_fails(cl_tab t, const uint4 v) {
    const uint32_t op = t[0];
    const cl_u32x4 a = *(cl_tab4)(t + 4), b = *(cl_tab4)(t + 8);
    const bool range = (v.x >= a.x) & (v.x <= b.x);
    bool eq = (v.x & b.x) == a.x;
    if (WIDE) eq = eq & ((v.y & b.y) == a.y) & ((v.z & b.z) == a.z) & ((v.w & b.w) == a.w);
    const bool m = op >= ZP_SEL_RANGE ? range : eq;      // uniform select
    return m == (bool)(op & 1u);             // MASK_NE, NOT_RANGE: the odd codes
}

// col_values' sink: the rules still alive, W dwords of them.
template <int W>
struct ClsSink {
    cl_tab tab;
    uint32_t nrules, colmask;
    uint32_t alive[W];
    uint32_t seen;                 // byte-array columns handed in
    static constexpr bool kStore = false;
    __device__ __forceinline__ bool l3() const { return (colmask & CL_COLS_L3) != 0; }
    __device__ __forceinline__ bool inner() const { return (colmask & CL_COLS_INNER) != 0; }
    __device__ __forceinline__ bool l4() const { return (colmask & CL_COLS_L4) != 0; }
    __device__ __forceinline__ bool wants(int col) const { return (colmask >> col) & 1u; }
    template <bool WIDE>
    __device__ __forceinline__ void value(int col, const uint4 v) {
        const uint32_t first = tab[CT_OFF_COLS(nrules) + 2 * col];
        const uint32_t cnt = tab[CT_OFF_COLS(nrules) + 2 * col + 1];
        cl_tab t = tab + CT_OFF_TERMS(nrules) + CT_TERM * first;
        // four terms' operands in flight: a column with many terms waits on the
        // scalar loads, not on the compares
#pragma unroll 4
        for (uint32_t k = 0; k < cnt; ++k, t += CT_TERM) {               // wave-uniform
            const bool fail = cl_term_fails<WIDE>(t, v);
            uint32_t set[W];
#pragma unroll
            for (int w = 0; w < W; w += 2) {           // W is even: 8-B loads
                set[w] = t[12 + w];
                set[w + 1] = t[13 + w];
            }
#pragma unroll
            for (int w = 0; w < W; ++w) alive[w] &= fail ? ~set[w] : ~0u;
        }
    }
    // The all-zero value of a byte-array column that was not handed in.
    __device__ __forceinline__ void absent(int col) {
        if (!wants(col)) return;
        const bool miss = !((seen >> col) & 1u);
#pragma unroll
        for (int w = 0; w < W; ++w)
            alive[w] &= miss ? ~tab[CT_OFF_ZERO(nrules) + CT_SETW * col + w] : ~0u;
    }
    template <class R>
    __device__ __forceinline__ void mac(int col, R& rd, uint32_t x) {        // as col_mac
        if (!wants(col)) return;
        uint4 v = make_uint4(0, 0, 0, 0);
        v.x = rd_le(rd, x, 2);
        v.x |= rd_le(rd, x + 2, 2) << 16;
        v.y = rd_le(rd, x + 4, 2);
        seen |= 1u << col;
        value<true>(col, v);
    }
    template <class R>
    __device__ __forceinline__ void addr(int col, R& rd, uint32_t x, bool v6) {   // as col_addr
        if (!wants(col)) return;
        uint4 v;
        v.x = rd_le(rd, x, 4);
        v.y = v6 ? rd_le(rd, x + 4, 4) : 0u;
        v.z = v6 ? rd_le(rd, x + 8, 4) : 0u;
        v.w = v6 ? rd_le(rd, x + 12, 4) : 0u;
        seen |= 1u << col;
        value<true>(col, v);
    }
    template <typename T>
    __device__ __forceinline__ void put(int col, T v) {
        if (wants(col)) value<false>(col, make_uint4((uint32_t)v, 0, 0, 0));
    }
};

// Sum of a u32 over the wave, exact in 64 bits (two 16-bit halves).
__device__ __forceinline__ uint64_t cl_wave_sum(uint32_t v) {
    uint32_t lo = v & 0xFFFFu, hi = v >> 16;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo += __shfl_xor(lo, o);
        hi += __shfl_xor(hi, o);
    }
    return ((uint64_t)hi << 16) + lo;
}

// W: dwords of the alive set. TERMS: the frames may be read (the table says
// whether they are); without it the kernel streams records and lens only and
// a table with terms is refused through `status`.
template <int W, bool TERMS>
__global__ void __launch_bounds__(CL_BLOCK, 5)         // five workgroups per CU: what the LDS allows
zp_classify_kernel(const uint8_t* __restrict__ arena, const uint64_t* __restrict__ offs,
                   const uint32_t* __restrict__ lens, const zp_record* __restrict__ recs, uint64_t n,
                   const uint32_t* __restrict__ table, uint32_t nrules, ClsAccept acc,
                   uint32_t* __restrict__ rule_of, zp_rule_hits* __restrict__ hits,
                   uint64_t* __restrict__ mask, uint64_t* __restrict__ status) {
    __shared__ uint4 win[TERMS ? FX_CH * FX_BLOCK : 1];
    // the workgroup's counters: packets fit 32 bits (n < 2^32), which keeps the
    // workgroup within 32 KiB of LDS (five workgroups per CU beside the window)
    __shared__ unsigned long long hbytes[ZP_CLASSIFY_MAX_RULES + 1];
    __shared__ uint32_t hpkts[ZP_CLASSIFY_MAX_RULES + 1];
    cl_tab tab = (cl_tab)(uintptr_t)table;
    // The header first: nothing behind it is read unless it is this table's.
    const uint32_t flags = tab[CT_H_FLAGS];
    const bool good = tab[CT_H_MAGIC] == CT_MAGIC && tab[CT_H_VERSION] == CT_VERSION &&
        tab[CT_H_NRULES] == nrules && tab[CT_H_BYTES] == 4u * CT_WORDS(nrules) &&
        (TERMS || !(flags & CT_F_TERMS)) && (lens || !(flags & CT_F_BOUNDED));
    if (blockIdx.x == 0 && threadIdx.x == 0) *status = good ? 0 : 1;
    if (!good || n == 0) return;                       // uniform over the grid

    const uint32_t lane = threadIdx.x & 63;
    if (hits) {
        for (uint32_t k = threadIdx.x; k <= nrules; k += CL_BLOCK) {
            hbytes[k] = 0;
            hpkts[k] = 0;
        }
        __syncthreads();
    }
    const uint32_t colmask = tab[CT_H_COLMASK], npreds = tab[CT_H_NPREDS];
    // A workgroup takes tiles blockIdx.x, + gridDim.x, ...: its counters gather
    // in LDS over all of them. A wave stages and reads only its own cells of
    // the window, so the tiles need no barrier between them.
    const uint64_t ntiles = (n + CL_BLOCK - 1) / CL_BLOCK;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t i0 = tile * CL_BLOCK + threadIdx.x;
        // Lanes past the batch stay for the cooperative staging and the ballot.
        const bool live = i0 < n;
        const uint64_t i = live ? i0 : n - 1;
        const zp_u32x2 q = *(const FX_GLOBAL zp_u32x2*)(recs + i);
        const uint32_t ln = lens ? lens[i] : 0u;

        ClsSink<W> s;
        s.tab = tab;
        s.nrules = nrules;
        s.colmask = colmask;
        s.seen = 0;
#pragma unroll
        for (int w = 0; w < W; ++w) {
            const uint32_t left = nrules > 32u * w ? nrules - 32u * w : 0u;
            s.alive[w] = !live ? 0u : left >= 32 ? ~0u : (1u << left) - 1u;
        }
        // The record predicates: flags, err (the record's first word) and the length.
        {
            const uint32_t f = q.x & ZP_F_MASK, e = q.x >> 26;
            cl_tab p = tab + CT_OFF_PREDS;
            for (uint32_t k = 0; k < npreds; ++k, p += CT_PRED) {        // wave-uniform
                const cl_u32x4 p0 = *(cl_tab4)p, p1 = *(cl_tab4)(p + 4);
                const uint32_t all = p0.x, any = p0.y, none = p0.z, mn = p1.x, mx = p1.y;
                const int32_t err = (int32_t)p0.w;
                bool ok = ((f & all) == all) & ((f & none) == 0) & ((any == 0) | ((f & any) != 0));
                ok = ok & ((err == ZP_SEL_ERR_ANY) |
                           (err == ZP_SEL_ERR_NONZERO ? e != 0 : e == (uint32_t)err));
                ok = ok & ((lens == nullptr) | ((ln >= mn) & (ln <= mx)));
#pragma unroll
                for (int w = 0; w < W; ++w) s.alive[w] &= ok ? ~0u : ~p[8 + w];
            }
        }
        if (TERMS && (flags & CT_F_TERMS)) {           // uniform
            uint32_t any = 0;
#pragma unroll
            for (int w = 0; w < W; ++w) any |= s.alive[w];
            zp_rec_full r;
            const bool far = fx_rec_decode(q, r);      // zp_colrec.h
            // A frame no rule's predicate leaves in is not staged.
            const bool ok = any != 0 && r.err == 0 && (r.flags & ZP_F_ETHERNET);
            const uint32_t len = ok ? ln : 0u;
            const uintptr_t ga = (uintptr_t)arena + (ok ? offs[i] : 0);
            Hdr h;
            h.g = (const uint8_t*)ga;
            h.shift = (uint32_t)(ga & 15);
            // Stage only as far as the union of the rules' columns reads.
            uint32_t need = fx_rec_need(r, ok, far, s.l3(), s.inner(), s.l4());
            need = need < len ? need : len;
            h.wlen = need < FX_WIN - h.shift ? need : FX_WIN - h.shift;
            h.win = (const uint8_t*)&win[TERMS ? threadIdx.x : 0];
            h.xc = make_uint4(0, 0, 0, 0);
            h.xi = ~0u;
            fx_stage(win, ga, len, h);
            HdrReader rd{h};
            fx_rec_finish(rd, r, ok && (far || s.l3() || s.inner()), far);
            col_values(rd, r, ok, len, s);
            s.absent(ZP_COL_DEST_MAC);
            s.absent(ZP_COL_SRC_MAC);
            s.absent(ZP_COL_SRC_ADDR);
            s.absent(ZP_COL_DEST_ADDR);
            s.absent(ZP_COL_INNER_SRC_ADDR);
            s.absent(ZP_COL_INNER_DEST_ADDR);
            // the next tile's staging must not overtake this tile's reads of the window
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
        uint32_t rule = ZP_RULE_NONE;
#pragma unroll
        for (int w = W - 1; w >= 0; --w)
            if (s.alive[w]) rule = 32u * w + (uint32_t)__builtin_ctz(s.alive[w]);
        if (live && rule_of) rule_of[i0] = rule;
        const uint32_t slot = rule == ZP_RULE_NONE ? nrules : rule;   // its entry of hits / bit of accept
        if (mask) {
            uint32_t aw = 0;
#pragma unroll
            for (int k = 0; k <= W; ++k) aw = (slot >> 5) == (uint32_t)k ? acc.w[k] : aw;
            const uint64_t b = __ballot(live && ((aw >> (slot & 31)) & 1u));
            if (lane == 0 && live) mask[i0 >> 6] = b;  // i0: the wave's first frame
        }
        if (hits) {
            // The two most common cases first, each as one reduced pair from one
            // lane: the frames that share the first live lane's rule, then those
            // that share the next remaining lane's. What is left adds per lane.
            uint64_t rem = __ballot(live);
#pragma unroll
            for (int it = 0; it < 2; ++it) {
                if (!rem) break;                        // uniform over the wave
                const uint32_t lead = (uint32_t)__builtin_ctzll(rem);
                const uint32_t lslot = (uint32_t)__shfl((int)slot, (int)lead);
                const bool in = ((rem >> lane) & 1u) && slot == lslot;
                const uint64_t grp = __ballot(in);
                const uint64_t bytes = cl_wave_sum(in ? ln : 0u);
                if (lane == lead) {
                    atomicAdd(&hpkts[lslot], (uint32_t)__builtin_popcountll(grp));
                    atomicAdd(&hbytes[lslot], (unsigned long long)bytes);
                }
                rem &= ~grp;
            }
            if ((rem >> lane) & 1u) {
                atomicAdd(&hpkts[slot], 1u);
                atomicAdd(&hbytes[slot], (unsigned long long)ln);
            }
        }
    }
    if (hits) {
        __syncthreads();
        unsigned long long* const g = (unsigned long long*)hits;
        for (uint32_t k = threadIdx.x; k <= nrules; k += CL_BLOCK) {
            const unsigned long long pk = hpkts[k], by = hbytes[k];
            if (pk) atomicAdd(g + 2 * k, pk);
            if (by) atomicAdd(g + 2 * k + 1, by);
        }
    }
}

// ---- host ------------------------------------------------------------------
extern "C" uint64_t zp_classify_table_bytes(uint32_t nrules) {
    if (nrules == 0 || nrules > ZP_CLASSIFY_MAX_RULES) return 0;
    return 4ull * CT_WORDS(nrules);
}

struct CtTerm {                    // a distinct term while compiling
    uint32_t col, op, a[4], b[4], rules[CT_SETW];
};

static bool ct_term_holds(const CtTerm& t, const uint32_t v[4]) {
    const bool m = t.op >= ZP_SEL_RANGE
        ? v[0] >= t.a[0] && v[0] <= t.b[0]
        : (v[0] & t.b[0]) == t.a[0] && (v[1] & t.b[1]) == t.a[1] && (v[2] & t.b[2]) == t.a[2] &&
          (v[3] & t.b[3]) == t.a[3];
    return m != (bool)(t.op & 1u);
}

extern "C" int zp_classify_compile(const zp_select* rules, uint32_t nrules, void* table,
                                   uint64_t table_bytes) {
    char* const eb = zp__errbuf();
    if (!rules || !table) {
        snprintf(eb, 256, "zp_classify_compile: null rules or table");
        return -1;
    }
    if (nrules == 0 || nrules > ZP_CLASSIFY_MAX_RULES) {
        snprintf(eb, 256, "zp_classify_compile: nrules %u not in 1..ZP_CLASSIFY_MAX_RULES", nrules);
        return -1;
    }
    if (table_bytes < zp_classify_table_bytes(nrules)) {
        snprintf(eb, 256, "zp_classify_compile: table_bytes below zp_classify_table_bytes(%u)", nrules);
        return -1;
    }
    if ((uintptr_t)table & 3) {
        snprintf(eb, 256, "zp_classify_compile: misaligned table");
        return -1;
    }
    // Everything is checked before the first byte of `table` is written.
    for (uint32_t r = 0; r < nrules; ++r) {
        const zp_select& s = rules[r];
        if (s.nterms > ZP_SELECT_MAX_TERMS) {
            snprintf(eb, 256, "zp_classify_compile: rule %u: more than ZP_SELECT_MAX_TERMS terms", r);
            return -1;
        }
        for (uint32_t k = 0; k < s.nterms; ++k) {
            const zp_select_term& t = s.terms[k];
            const int w = zp_col_width(t.col);
            if (t.col >= ZP_COL_COUNT || w == 0) {
                snprintf(eb, 256, "zp_classify_compile: rule %u: term %u: column %u out of range", r, k, t.col);
                return -1;
            }
            if (t.op > ZP_SEL_NOT_RANGE) {
                snprintf(eb, 256, "zp_classify_compile: rule %u: term %u: unknown op %u", r, k, t.op);
                return -1;
            }
            for (int p = 0; p < 6; ++p)
                if (t.pad[p]) {
                    snprintf(eb, 256, "zp_classify_compile: rule %u: term %u: pad must be 0", r, k);
                    return -1;
                }
            if (t.op >= ZP_SEL_RANGE && w > 4) {
                snprintf(eb, 256, "zp_classify_compile: rule %u: term %u: RANGE on byte-array column %u",
                         r, k, t.col);
                return -1;
            }
        }
    }
    uint32_t* const T = (uint32_t*)table;
    memset(T, 0, (size_t)zp_classify_table_bytes(nrules));
    uint32_t flags = 0, colmask = 0, npreds = 0;
    // distinct predicates, in the order of their first rule
    uint32_t* const P = T + CT_OFF_PREDS;
    for (uint32_t r = 0; r < nrules; ++r) {
        const zp_select& s = rules[r];
        const uint32_t key[6] = {s.flags_all, s.flags_any, s.flags_none, (uint32_t)s.err, s.min_len,
                                 s.max_len};
        if (s.min_len != 0 || s.max_len != UINT32_MAX) flags |= CT_F_BOUNDED;
        uint32_t k = 0;
        while (k < npreds && memcmp(P + CT_PRED * k, key, sizeof key)) ++k;
        if (k == npreds) memcpy(P + CT_PRED * npreds++, key, sizeof key);
        P[CT_PRED * k + 8 + (r >> 5)] |= 1u << (r & 31);
    }
    // distinct terms, in the order of their first rule, then grouped by column
    std::vector<CtTerm> terms((size_t)nrules * ZP_SELECT_MAX_TERMS);
    uint32_t nt = 0;
    for (uint32_t r = 0; r < nrules; ++r) {
        const zp_select& s = rules[r];
        for (uint32_t k = 0; k < s.nterms; ++k) {
            const zp_select_term& t = s.terms[k];
            const int w = zp_col_width(t.col);
            CtTerm c;
            memset(&c, 0, sizeof c);
            c.col = t.col;
            c.op = t.op;
            memcpy(c.a, t.a, (size_t)w);               // the column's width, zeros behind
            memcpy(c.b, t.b, (size_t)w);
            uint32_t j = 0;
            while (j < nt && memcmp(&terms[j], &c, offsetof(CtTerm, rules))) ++j;
            if (j == nt) terms[nt++] = c;
            terms[j].rules[r >> 5] |= 1u << (r & 31);
            colmask |= 1u << t.col;
            flags |= CT_F_TERMS;
        }
    }
    uint32_t* const C = T + CT_OFF_COLS(nrules);
    uint32_t* const Z = T + CT_OFF_ZERO(nrules);
    uint32_t* D = T + CT_OFF_TERMS(nrules);
    uint32_t at = 0;
    const uint32_t zero[4] = {0, 0, 0, 0};
    for (uint32_t col = 0; col < ZP_COL_COUNT; ++col) {
        C[2 * col] = at;
        for (uint32_t j = 0; j < nt; ++j) {
            const CtTerm& c = terms[j];
            if (c.col != col) continue;
            D[0] = c.op;
            memcpy(D + 4, c.a, 16);
            memcpy(D + 8, c.b, 16);
            memcpy(D + 12, c.rules, 4 * CT_SETW);
            if (!ct_term_holds(c, zero))
                for (int w = 0; w < CT_SETW; ++w) Z[CT_SETW * col + w] |= c.rules[w];
            D += CT_TERM;
            ++at;
        }
        C[2 * col + 1] = at - C[2 * col];
    }
    T[CT_H_MAGIC] = CT_MAGIC;
    T[CT_H_VERSION] = CT_VERSION;
    T[CT_H_NRULES] = nrules;
    T[CT_H_FLAGS] = flags;
    T[CT_H_COLMASK] = colmask;
    T[CT_H_NPREDS] = npreds;
    T[CT_H_NTERMS] = nt;
    T[CT_H_BYTES] = 4u * CT_WORDS(nrules);
    return (flags & CT_F_TERMS) ? 1 : 0;
}

// Workgroups one CU holds: 160 KiB of LDS over 31 KiB with the window; 32
// waves over 4 without.
#define CL_WG_PER_CU_TERMS 5
#define CL_WG_PER_CU_REC 8

static int cl_compute_units() {
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

static int cl_fail(const char* what) {
    snprintf(zp__errbuf(), 256, "zp_classify_device: %s", what);
    return -1;
}

template <bool TERMS>
static void cl_launch(uint32_t words, unsigned blocks, hipStream_t st, const uint8_t* arena,
                      const uint64_t* offs, const uint32_t* lens, const zp_record* records,
                      uint64_t n, const uint32_t* table, uint32_t nrules, const ClsAccept& acc,
                      uint32_t* rule_of, zp_rule_hits* hits, uint64_t* mask, uint64_t* status) {
#define CL_GO(W)                                                                                   \
    hipLaunchKernelGGL((zp_classify_kernel<W, TERMS>), dim3(blocks), dim3(CL_BLOCK), 0, st, arena, \
                       offs, lens, records, n, table, nrules, acc, rule_of, hits, mask, status)
    if (words <= 2) CL_GO(2);
    else if (words <= 4) CL_GO(4);
    else if (words <= 6) CL_GO(6);
    else CL_GO(8);
#undef CL_GO
}

extern "C" int zp_classify_device(const uint8_t* arena, const uint64_t* offs, const uint32_t* lens,
                                  const zp_record* records, uint64_t n, const void* table,
                                  uint64_t table_bytes, uint32_t nrules, const uint64_t* accept,
                                  uint32_t* rule_of, zp_rule_hits* hits, uint64_t* mask,
                                  uint64_t* status, void* stream) {
    if (!records) return cl_fail("null records");
    if (!table) return cl_fail("null table");
    if (!status) return cl_fail("null status");
    if (nrules == 0 || nrules > ZP_CLASSIFY_MAX_RULES)
        return cl_fail("nrules not in 1..ZP_CLASSIFY_MAX_RULES");
    if (table_bytes < zp_classify_table_bytes(nrules))
        return cl_fail("table_bytes below zp_classify_table_bytes(nrules)");
    if (n >= (1ull << 32)) return cl_fail("rule_of holds 32-bit indices: n must be below 2^32");
    if (((uintptr_t)table & 7) || ((uintptr_t)hits & 7) || ((uintptr_t)mask & 7) ||
        ((uintptr_t)status & 7) || ((uintptr_t)rule_of & 3))
        return cl_fail("misaligned pointer");
    if (hits && !lens) return cl_fail("hits need lens");
    // arena == NULL and offs == NULL: the caller says the table is record-only
    // (zp_classify_compile returned 0); the kernel checks that against the header.
    const bool frames = arena || offs;
    if (frames && (!arena || !offs || !lens))
        return cl_fail("a table that reads frames needs arena, offs and lens");
    ClsAccept acc;
    memset(&acc, 0, sizeof acc);
    if (accept) {
        uint64_t a[(ZP_CLASSIFY_MAX_RULES + 64) / 64];
        memset(a, 0, sizeof a);
        memcpy(a, accept, 8 * (size_t)((nrules + 64) / 64));
        for (uint32_t k = 0; k <= nrules; ++k)
            if ((a[k >> 6] >> (k & 63)) & 1u) acc.w[k >> 5] |= 1u << (k & 31);
    } else {
        for (uint32_t k = 0; k < nrules; ++k) acc.w[k >> 5] |= 1u << (k & 31);
    }
    uint64_t tiles = n ? (n + CL_BLOCK - 1) / CL_BLOCK : 1;          // n == 0: status only
    // as many workgroups as the device holds at once (by LDS with the window,
    // by waves without), each walking several tiles
    const uint64_t fill = (uint64_t)cl_compute_units() * (frames ? CL_WG_PER_CU_TERMS : CL_WG_PER_CU_REC);
    if (tiles > fill) tiles = fill;
    const uint32_t words = (nrules + 31) / 32;
    if (frames)
        cl_launch<true>(words, (unsigned)tiles, (hipStream_t)stream, arena, offs, lens, records, n,
                        (const uint32_t*)table, nrules, acc, rule_of, hits, mask, status);
    else
        cl_launch<false>(words, (unsigned)tiles, (hipStream_t)stream, arena, offs, lens, records, n,
                         (const uint32_t*)table, nrules, acc, rule_of, hits, mask, status);
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return 0;
    snprintf(zp__errbuf(), 256, "zp_classify_kernel launch: %s", hipGetErrorString(e));
    return -2;
}
