/* zp_route.h — the compiled route table (include/zero_packet.h,
 * zp_route_compile) and the walk over it. Plain C: the host side
 * (zp_route_tab.c) and the kernel (zp_route.hip) compile the same functions,
 * so zp_route_lookup_host runs the very walk the device runs.
 *
 * The table is dwords:
 *   header  RT_HDR dwords: signature, format version, prefixes, nodes, the
 *           table's bytes (two dwords), zeros;
 *   roots   one per IP version (4, then 6): RT_ROOT entries indexed by the
 *           address's first 16 bits;
 *   nodes   RT_NODE entries each, indexed by the address's next 8 bits.
 * An entry is a leaf (bit 31 clear: the value of the longest prefix that
 * covers every address that reaches it, or RT_LEAF_NONE) or a child (bit 31
 * set, the node's index in the low bits). Leaves are pushed: a lookup never
 * remembers a shorter match, the entry it ends on is the answer. IPv4 ends
 * after at most 3 entries, IPv6 after at most 15.
 *
 * The walk is safe on any body behind a header that passed rt_header_ok: it
 * makes at most RT_STEPS_V4 / RT_STEPS_V6 loads, and a child index at or past
 * the header's node count ends it with ZP_ROUTE_NONE, so nothing loops and
 * nothing outside [table, table + bytes) is read.
 */
#pragma once
#include <stdint.h>

#include "../../include/zero_packet.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RT_FN __host__ __device__ static inline __attribute__((always_inline))
#else
#define RT_FN static inline
#endif

#define RT_MAGIC 0x5452505Au        /* "ZPRT" */
#define RT_VERSION 1u
#define RT_HDR 16                   /* dwords */
#define RT_H_MAGIC 0
#define RT_H_VERSION 1
#define RT_H_PREFIXES 2
#define RT_H_NODES 3
#define RT_H_BYTES_LO 4
#define RT_H_BYTES_HI 5
#define RT_ROOT 65536u              /* entries of a root: a 16-bit stride */
#define RT_NODE 256u                /* entries of a node: 8-bit strides */
#define RT_OFF_ROOT4 RT_HDR
#define RT_OFF_ROOT6 (RT_HDR + RT_ROOT)
#define RT_OFF_NODES (RT_HDR + 2u * RT_ROOT)
#define RT_CHILD 0x80000000u
#define RT_LEAF_NONE 0x7FFFFFFFu    /* ZP_ROUTE_VALUE_MAX + 1: no prefix covers this entry */
#define RT_STEPS_V4 3               /* root, bytes 2 and 3 */
#define RT_STEPS_V6 15              /* root, bytes 2 to 15 */

/* Bytes of a table with `nodes` nodes. */
RT_FN uint64_t rt_bytes(uint64_t nodes) { return 4ull * RT_OFF_NODES + 4ull * RT_NODE * nodes; }

/* Whether h[0, RT_HDR) is the header of a table of exactly table_bytes bytes;
 * reads the header only. */
RT_FN int rt_header_ok(const uint32_t* h, uint64_t table_bytes) {
    const uint64_t bytes = ((uint64_t)h[RT_H_BYTES_HI] << 32) | h[RT_H_BYTES_LO];
    return h[RT_H_MAGIC] == RT_MAGIC && h[RT_H_VERSION] == RT_VERSION && bytes == table_bytes &&
           bytes == rt_bytes(h[RT_H_NODES]);
}

/* The walk over table T (its header checked by the caller). a: the address
 * as the address columns hold it, in little-endian dwords; version 4 reads
 * a[0] only. A version other than 4 or 6 makes no load. */
RT_FN uint32_t rt_lookup(const uint32_t* T, uint32_t nodes, const uint32_t a[4], uint32_t version) {
    if (version != 4 && version != 6) return ZP_ROUTE_NONE;
    const int v6 = version == 6;
    /* the address bytes not yet consumed, lowest byte next */
    uint64_t lo = ((uint64_t)(v6 ? a[1] : 0u) << 32) | a[0];
    uint64_t hi = v6 ? (((uint64_t)a[3] << 32) | a[2]) : 0u;
    const uint32_t first = (((uint32_t)lo & 0xFFu) << 8) | (((uint32_t)lo >> 8) & 0xFFu);
    lo = (lo >> 16) | (hi << 48);
    hi >>= 16;
    uint32_t e = T[(v6 ? RT_OFF_ROOT6 : RT_OFF_ROOT4) + first];
    for (int left = (v6 ? RT_STEPS_V6 : RT_STEPS_V4) - 1; left > 0 && (e & RT_CHILD); --left) {
        const uint32_t node = e & ~RT_CHILD;
        if (node >= nodes) return ZP_ROUTE_NONE;            /* not a compiled body */
        e = T[RT_OFF_NODES + (uint64_t)node * RT_NODE + ((uint32_t)lo & 0xFFu)];
        lo = (lo >> 8) | (hi << 56);
        hi >>= 8;
    }
    if (e & RT_CHILD) return ZP_ROUTE_NONE;                 /* a child where the address ends */
    return e == RT_LEAF_NONE ? ZP_ROUTE_NONE : e;
}
