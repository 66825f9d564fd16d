/* The host side of the route stage as a stand-alone program, for a build
 * under -fsanitize=address,undefined (tests/test_routes.py builds it together
 * with zero-packet_amd/csrc/zp_route_tab.c and runs it):
 *   - tables of nested chains with every length of interest, compiled from
 *     several orders into exactly sized heap buffers: the same bytes;
 *   - zp_route_lookup_host against a brute-force longest-prefix match on the
 *     prefixes' first and last addresses, their neighbours and random ones;
 *   - every refusal leaves the table untouched;
 *   - a body of random dwords, of children only, of one self-pointing node,
 *     behind a valid header, at the end of an exactly sized allocation.
 * Prints "route_host: OK" and returns 0, or says what differed. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "zero_packet.h"

static char errbuf[256];
char* zp__errbuf(void) { return errbuf; }

static const uint8_t LENS4[] = {0, 1, 15, 16, 17, 23, 24, 25, 31, 32};
static const uint8_t LENS6[] = {0, 1, 16, 17, 24, 63, 64, 65, 120, 121, 127, 128};

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(void) {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 32);
}

#define FAIL(...)                                   \
    do {                                            \
        printf("route_host: " __VA_ARGS__);         \
        printf("\n");                               \
        exit(1);                                    \
    } while (0)

static int covers(const zp_route_prefix* p, const uint8_t a[16], int version) {
    if (p->version != version) return 0;
    for (uint32_t bit = 0; bit < p->len; ++bit)
        if ((p->addr[bit >> 3] ^ a[bit >> 3]) & (0x80u >> (bit & 7))) return 0;
    return 1;
}

static uint32_t brute(const zp_route_prefix* p, uint32_t n, const uint8_t a[16], int version) {
    uint32_t best = ZP_ROUTE_NONE;
    int len = -1;
    for (uint32_t k = 0; k < n; ++k)
        if (covers(p + k, a, version) && (int)p[k].len > len) {
            len = p[k].len;
            best = p[k].value;
        }
    return best;
}

/* addr truncated to len bits, unless the table has it already */
static uint32_t add(zp_route_prefix* p, uint32_t n, int version, const uint8_t addr[16], uint32_t len) {
    zp_route_prefix q;
    memset(&q, 0, sizeof q);
    for (uint32_t bit = 0; bit < len; ++bit) q.addr[bit >> 3] |= addr[bit >> 3] & (0x80u >> (bit & 7));
    q.len = (uint8_t)len;
    q.version = (uint8_t)version;
    q.value = 100 + n;
    for (uint32_t k = 0; k < n; ++k)
        if (p[k].version == q.version && p[k].len == q.len && !memcmp(p[k].addr, q.addr, 16)) return n;
    p[n] = q;
    return n + 1;
}

static void check_lookups(const zp_route_prefix* p, uint32_t n, const void* table, uint64_t bytes) {
    uint32_t checked = 0;
    for (uint32_t k = 0; k < n; ++k) {
        const int version = p[k].version, nb = version == 4 ? 4 : 16;
        uint8_t lo[16], hi[16], a[16];
        memcpy(lo, p[k].addr, 16);
        memcpy(hi, p[k].addr, 16);
        for (int bit = p[k].len; bit < 8 * nb; ++bit) hi[bit >> 3] |= (uint8_t)(0x80u >> (bit & 7));
        for (int which = 0; which < 4; ++which) {
            memcpy(a, which & 1 ? hi : lo, 16);
            if (which >= 2) {                       /* the neighbour just outside: -1 / +1 */
                int carry = 1;
                for (int b = nb - 1; b >= 0 && carry; --b) {
                    if (which == 2) carry = a[b]-- == 0;
                    else carry = ++a[b] == 0;
                }
                if (carry) continue;                /* wrapped round: there is no neighbour */
            }
            for (int v = 4; v <= 6; v += 2) {       /* and the same bytes under the other version */
                uint8_t q[16];
                memcpy(q, a, 16);
                if (v == 4) memset(q + 4, 0, 12);
                const uint32_t got = zp_route_lookup_host(table, bytes, q, v), want = brute(p, n, q, v);
                if (got != want) FAIL("prefix %u, address %d, version %d: %u, expected %u", k, which, v, got, want);
                ++checked;
            }
        }
    }
    for (uint32_t k = 0; k < 4000; ++k) {
        uint8_t a[16];
        for (int b = 0; b < 16; ++b) a[b] = (uint8_t)rnd();
        const int v = k & 1 ? 6 : 4;
        if (v == 4) memset(a + 4, 0, 12);
        if (zp_route_lookup_host(table, bytes, a, v) != brute(p, n, a, v)) FAIL("random address %u", k);
    }
    if (zp_route_lookup_host(table, bytes, p[0].addr, 5) != ZP_ROUTE_NONE) FAIL("version 5 matched");
    if (checked < 6 * n) FAIL("too few addresses checked");
}

int main(void) {
    enum { CAP = 1024 };
    zp_route_prefix* p = calloc(CAP, sizeof *p);
    zp_route_prefix* q = calloc(CAP, sizeof *q);
    if (!p || !q) return 2;
    uint32_t n = 0;
    /* nested chains: 10.0.0.1 and a00:1::1 (the aliasing pair), the extremes, random addresses */
    uint8_t seeds[12][16] = {{10, 0, 0, 1}, {0x0a, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1}, {0}, {0}};
    memset(seeds[2], 0xFF, 16);
    for (int s = 4; s < 12; ++s)
        for (int b = 0; b < 16; ++b) seeds[s][b] = (uint8_t)rnd();
    for (int s = 0; s < 12; ++s) {
        for (size_t k = 0; k < sizeof LENS4; ++k) n = add(p, n, 4, seeds[s], LENS4[k]);
        for (size_t k = 0; k < sizeof LENS6; ++k) n = add(p, n, 6, seeds[s], LENS6[k]);
    }
    if (n < 150 || n > CAP) FAIL("%u prefixes", n);

    const uint64_t bytes = zp_route_table_bytes(p, n);
    uint64_t levels = 0;
    for (uint32_t k = 0; k < n; ++k) levels += p[k].len <= 16 ? 0 : (p[k].len - 16 + 7) / 8;
    if (bytes == 0 || bytes > 64 + (512u << 10) + 1024 * levels) FAIL("size %llu: %s", (unsigned long long)bytes, errbuf);
    uint8_t* first = NULL;
    for (int round = 0; round < 5; ++round) {
        memcpy(q, p, n * sizeof *p);
        for (uint32_t k = n - 1; round && k > 0; --k) {             /* a shuffle */
            const uint32_t j = rnd() % (k + 1);
            const zp_route_prefix t = q[k];
            q[k] = q[j];
            q[j] = t;
        }
        for (int fill = 0; fill < 2; ++fill) {
            uint8_t* t = malloc(bytes);                             /* exactly sized */
            if (!t) return 2;
            memset(t, fill ? 0xA5 : 0x00, bytes);
            if (zp_route_table_bytes(q, n) != bytes) FAIL("size differs with the order");
            if (zp_route_compile(q, n, t, bytes) != 0) FAIL("compile: %s", errbuf);
            if (!first) first = t;
            else {
                if (memcmp(first, t, bytes)) FAIL("round %d fill %d: other bytes", round, fill);
                free(t);
            }
        }
    }
    check_lookups(p, n, first, bytes);

    /* the empty table */
    {
        const uint64_t eb = zp_route_table_bytes(NULL, 0);
        uint8_t* t = malloc(eb);
        if (!t || eb != 64 + (512u << 10) || zp_route_compile(NULL, 0, t, eb) != 0) FAIL("empty table");
        if (zp_route_lookup_host(t, eb, seeds[0], 4) != ZP_ROUTE_NONE) FAIL("empty table matched");
        free(t);
    }

    /* refusals: the table stays as it was */
    {
        uint8_t* t = malloc(bytes);
        if (!t) return 2;
        memset(t, 0x5A, bytes);
        memcpy(q, p, n * sizeof *p);
        q[7].version = 5;
        int bad = zp_route_compile(q, n, t, bytes) >= 0;
        memcpy(q, p, n * sizeof *p);
        q[9] = q[3];
        bad |= zp_route_compile(q, n, t, bytes) >= 0 || !strstr(errbuf, "prefixes 3 and 9");
        bad |= zp_route_compile(p, n, t, bytes - 1) >= 0;
        bad |= zp_route_compile(p, ZP_ROUTE_MAX_PREFIXES + 1, t, bytes) >= 0;
        for (uint64_t k = 0; k < bytes; ++k) bad |= t[k] != 0x5A;
        if (bad) FAIL("a refused compile: %s", errbuf);
        free(t);
    }

    /* a body that is not a compiled one, behind the valid header */
    {
        uint32_t* t = malloc(bytes);
        if (!t) return 2;
        const uint32_t nodes = ((const uint32_t*)(const void*)first)[3];
        for (int fill = 0; fill < 4; ++fill) {
            memcpy(t, first, bytes);
            for (uint64_t k = 16; k < bytes / 4; ++k)
                t[k] = fill == 0 ? rnd() : fill == 1 ? 0x80000000u | (rnd() % (4 * nodes))
                    : fill == 2 ? 0x80000000u | (nodes - 1) : 0x80000000u;
            for (uint32_t k = 0; k < 20000; ++k) {
                uint8_t a[16];
                for (int b = 0; b < 16; ++b) a[b] = (uint8_t)rnd();
                const uint32_t got = zp_route_lookup_host(t, bytes, a, k & 1 ? 6 : 4);
                if (fill && got != ZP_ROUTE_NONE) FAIL("fill %d: a walk without a leaf gave %u", fill, got);
            }
        }
        memcpy(t, first, bytes);
        if (zp_route_lookup_host(t, bytes - 1024, seeds[0], 4) != ZP_ROUTE_NONE) FAIL("wrong size accepted");
        free(t);
    }
    free(first);
    free(p);
    free(q);
    printf("route_host: OK\n");
    return 0;
}
