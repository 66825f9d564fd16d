/*
 * zp_route_tab.c — the host side of the route stage (include/zero_packet.h):
 *
 *   zp_route_table_bytes   the exact size of a prefix set's compiled table
 *   zp_route_compile       the leaf-pushed multibit trie of zp_route.h
 *   zp_route_lookup_host   one address through the walk the kernel runs
 *
 * The prefixes are sorted by (version, addr, len). In that order a prefix
 * that covers another comes before it, which is all leaf pushing needs: the
 * entries a prefix fills are leaves (a child there would belong to a longer
 * prefix inside it, which comes later), and a new node starts as 256 copies
 * of the leaf it replaces, the best cover so far. The same order makes the
 * nodes a depth-first numbering (a subtree's nodes are adjacent) and lets
 * one pass over the sorted prefixes count them without building anything.
 * The order does not depend on the caller's, so neither do the bytes.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "zp_route.h"

char* zp__errbuf(void);

typedef struct rt_item {           /* a prefix while compiling: the sort key first */
    uint8_t version, addr[16], len;
    uint8_t pad[2];
    uint32_t value, index;         /* index: its place in the caller's array */
} rt_item;

static int rt_item_cmp(const void* x, const void* y) {
    return memcmp(x, y, 18);       /* version, addr, len */
}

/* Levels of nodes under the root a prefix of length len passes through:
 * ceil((len - 16) / 8), 0 up to /16. */
static uint32_t rt_levels(uint32_t len) { return len <= 16 ? 0u : (len - 16 + 7) / 8; }

/* Validates p[0, n) and returns them sorted (malloc'd; NULL with *bad = 1 on
 * a refusal, the cause in the error buffer under `fn`; NULL with *bad = 0
 * for n == 0) and the number of nodes of their trie. */
static rt_item* rt_prepare(const char* fn, const zp_route_prefix* p, uint32_t n, uint64_t* nodes,
                           int* bad) {
    char* const eb = zp__errbuf();
    *bad = 1;
    *nodes = 0;
    if (n > ZP_ROUTE_MAX_PREFIXES) {
        snprintf(eb, 256, "%s: %u prefixes, above ZP_ROUTE_MAX_PREFIXES", fn, n);
        return NULL;
    }
    if (n && !p) {
        snprintf(eb, 256, "%s: null prefixes", fn);
        return NULL;
    }
    for (uint32_t i = 0; i < n; ++i) {
        const zp_route_prefix* q = p + i;
        const uint32_t width = q->version == 4 ? 32u : 128u;
        if (q->version != 4 && q->version != 6) {
            snprintf(eb, 256, "%s: prefix %u: version %u is not 4 or 6", fn, i, q->version);
            return NULL;
        }
        if (q->len > width) {
            snprintf(eb, 256, "%s: prefix %u: len %u past the %u bits of version %u", fn, i, q->len,
                     width, q->version);
            return NULL;
        }
        if (q->pad[0] || q->pad[1]) {
            snprintf(eb, 256, "%s: prefix %u: pad must be 0", fn, i);
            return NULL;
        }
        if (q->value > ZP_ROUTE_VALUE_MAX) {
            snprintf(eb, 256, "%s: prefix %u: value above ZP_ROUTE_VALUE_MAX", fn, i);
            return NULL;
        }
        for (uint32_t k = 0; k < 16; ++k) {
            const uint32_t keep = q->len >= 8 * (k + 1) ? 0xFFu
                : q->len <= 8 * k ? 0u : (0xFF00u >> (q->len - 8 * k)) & 0xFFu;
            if (q->addr[k] & ~keep) {
                snprintf(eb, 256, "%s: prefix %u: address bits set past len %u (byte %u)", fn, i,
                         q->len, k);
                return NULL;
            }
        }
    }
    if (n == 0) {
        *bad = 0;
        return NULL;
    }
    rt_item* const s = (rt_item*)malloc((size_t)n * sizeof *s);
    if (!s) {
        snprintf(eb, 256, "%s: out of host memory for %u prefixes", fn, n);
        return NULL;
    }
    for (uint32_t i = 0; i < n; ++i) {
        s[i].version = p[i].version;
        memcpy(s[i].addr, p[i].addr, 16);
        s[i].len = p[i].len;
        s[i].pad[0] = s[i].pad[1] = 0;
        s[i].value = p[i].value;
        s[i].index = i;
    }
    qsort(s, n, sizeof *s, rt_item_cmp);
    for (uint32_t i = 1; i < n; ++i)
        if (!rt_item_cmp(s + i - 1, s + i)) {
            const uint32_t a = s[i - 1].index, b = s[i].index;
            snprintf(eb, 256, "%s: prefixes %u and %u are the same (version, len, addr)", fn,
                     a < b ? a : b, a < b ? b : a);
            free(s);
            return NULL;
        }
    /* The nodes: `open` levels of the previous prefixes' path are still on
     * this prefix's path as far as the two addresses share whole bytes. */
    uint32_t open = 0;                              /* levels open under root bytes 0-1 */
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t shared = 0;                        /* levels of the open path this one shares */
        if (i && s[i].version == s[i - 1].version) {
            uint32_t c = 0;
            while (c < 16 && s[i].addr[c] == s[i - 1].addr[c]) ++c;
            shared = c >= 2 ? c - 1 : 0;            /* level j hangs under bytes [0, j + 1) */
        }
        if (open > shared) open = shared;
        const uint32_t need = rt_levels(s[i].len);
        if (need > open) {
            *nodes += need - open;
            open = need;
        }
    }
    *bad = 0;
    return s;
}

uint64_t zp_route_table_bytes(const zp_route_prefix* p, uint32_t n) {
    uint64_t nodes;
    int bad;
    free(rt_prepare("zp_route_table_bytes", p, n, &nodes, &bad));
    return bad ? 0 : rt_bytes(nodes);
}

int zp_route_compile(const zp_route_prefix* p, uint32_t n, void* table, uint64_t table_bytes) {
    static const char fn[] = "zp_route_compile";
    char* const eb = zp__errbuf();
    if (!table) {
        snprintf(eb, 256, "%s: null table", fn);
        return -1;
    }
    if ((uintptr_t)table & 3) {
        snprintf(eb, 256, "%s: misaligned table", fn);
        return -1;
    }
    uint64_t nodes;
    int bad;
    rt_item* const s = rt_prepare(fn, p, n, &nodes, &bad);
    if (bad) return -1;
    const uint64_t bytes = rt_bytes(nodes);
    if (table_bytes < bytes) {                      /* nodes < 2^31: at most 14 per prefix */
        snprintf(eb, 256, "%s: table_bytes %llu below zp_route_table_bytes (%llu)", fn,
                 (unsigned long long)table_bytes, (unsigned long long)bytes);
        free(s);
        return -1;
    }
    /* Everything is checked: from here on `table` is written. */
    uint32_t* const T = (uint32_t*)table;
    memset(T, 0, 4 * RT_HDR);
    for (uint32_t k = 0; k < 2 * RT_ROOT; ++k) T[RT_OFF_ROOT4 + k] = RT_LEAF_NONE;
    uint32_t made = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const rt_item* q = s + i;
        const uint32_t first = ((uint32_t)q->addr[0] << 8) | q->addr[1];
        uint32_t* e = T + (q->version == 6 ? RT_OFF_ROOT6 : RT_OFF_ROOT4) + first;
        uint32_t bits = 16, at = 2;                 /* the stride at e, the address byte behind it */
        for (uint32_t lv = rt_levels(q->len); lv > 0; --lv, ++at) {
            if (!(*e & RT_CHILD)) {                 /* push the leaf down into a new node */
                uint32_t* const node = T + RT_OFF_NODES + (uint64_t)made * RT_NODE;
                for (uint32_t k = 0; k < RT_NODE; ++k) node[k] = *e;
                *e = RT_CHILD | made++;
            }
            e = T + RT_OFF_NODES + (uint64_t)(*e & ~RT_CHILD) * RT_NODE + q->addr[at];
            bits = 8;
        }
        /* the prefix ends inside this stride: it fills 2^k entries */
        const uint32_t used = q->len <= 16 ? q->len : q->len - 8 * (at - 1);
        const uint32_t span = 1u << (bits - used);
        for (uint32_t k = 0; k < span; ++k) e[k] = q->value;
    }
    free(s);
    if (made != nodes) {                            /* the count and the build disagree: a bug here */
        snprintf(eb, 256, "%s: internal: %u nodes built, %llu counted", fn, made,
                 (unsigned long long)nodes);
        return -3;
    }
    T[RT_H_MAGIC] = RT_MAGIC;
    T[RT_H_VERSION] = RT_VERSION;
    T[RT_H_PREFIXES] = n;
    T[RT_H_NODES] = (uint32_t)nodes;
    T[RT_H_BYTES_LO] = (uint32_t)bytes;
    T[RT_H_BYTES_HI] = (uint32_t)(bytes >> 32);
    return 0;
}

uint32_t zp_route_lookup_host(const void* table, uint64_t table_bytes, const uint8_t addr[16],
                              int version) {
    if (!table || !addr || ((uintptr_t)table & 3) || table_bytes < 4 * RT_HDR) return ZP_ROUTE_NONE;
    const uint32_t* const T = (const uint32_t*)table;
    if (!rt_header_ok(T, table_bytes)) return ZP_ROUTE_NONE;
    uint32_t a[4] = {0, 0, 0, 0};
    for (uint32_t k = 0; k < (version == 6 ? 16u : 4u); ++k) a[k >> 2] |= (uint32_t)addr[k] << (8 * (k & 3));
    return rt_lookup(T, T[RT_H_NODES], a, (uint32_t)version);
}
