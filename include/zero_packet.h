/*
 * zero_packet.h — C ABI of the MI355X-native batched PacketParser::parse.
 *
 * This is the drop-in boundary for zero-packet's parse path
 * (/root/reference/src/packet/parser.rs:53). The reference has no FFI of its
 * own; its boundary is the Rust API
 *
 *     pub fn PacketParser::parse(bytes: &'a [u8]) -> Result<PacketParser<'a>, &'static str>
 *
 * whose result is nine `Option<Reader>` fields (parser.rs:22-32). Every
 * reader is a sub-slice `&frame[start..]` that runs to the end of the frame,
 * so a parsed packet is fully described by header START OFFSETS. One
 * zp_record per frame carries those offsets plus presence bits, so a caller
 * (C++ facade include/zero_packet.hpp, the Rust shim in INTEGRATION.md) can
 * rebuild every reader without re-parsing.
 *
 * Plain pointers and sizes only; no torch types. Device pointers are HIP
 * device memory; hipStream_t is passed as void*.
 */
#ifndef ZERO_PACKET_H
#define ZERO_PACKET_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZP_ABI_VERSION 6   /* 2: 16-B record, extension chains in the ext side array;
                              3: reader-accessor error codes 36-37 (ZP_ERR_COUNT 38,
                                 ZP_STATS_COUNT 62), standalone readers and the
                                 checksum primitives (zp_reader_new, zp_*checksum*);
                              4: 8-B record (flags word + packed offsets); the IPv6
                                 final next header of a chain in its ext entry;
                              5: the far-L4 form (Ethernet code 3, the whole L4
                                 offset in `offs`) replaces v4's saturation at
                                 ZP_L4_FAR; zp_rec_decode;
                              6: the inline outer chain (ZP_CHAIN_INLINE): a short
                                 RFC-ordered IPv6 extension chain of a frame without
                                 ip_in_ip lives in the record, no ext entry */

/* ------------------------------------------------------------------------- */
/* Per-packet parse error codes. One code per DISTINCT reference error string */
/* (identical strings collapse: icmpv4.rs:94 == icmpv6.rs:91). zp_err_str()   */
/* returns the exact reference string. Codes marked (unreachable) cannot be   */
/* produced by parse() because an earlier check subsumes them; they exist so  */
/* the per-reader views can report them.                                      */
/* ------------------------------------------------------------------------- */
typedef enum zp_err {
    ZP_OK = 0,
    ZP_ERR_ETH_FRAME_TOO_SHORT = 1,   /* parser.rs:160                          */
    ZP_ERR_ETH_SLICE_TOO_SHORT = 2,   /* ethernet.rs:143 (unreachable)          */
    ZP_ERR_ETH_VLAN_TOO_SHORT = 3,    /* ethernet.rs:160 (unreachable)          */
    ZP_ERR_ETH_QINQ_TOO_SHORT = 4,    /* ethernet.rs:167 (unreachable)          */
    ZP_ERR_ETH_INVALID_QINQ = 5,      /* ethernet.rs:172                        */
    ZP_ERR_ARP_TOO_SHORT = 6,         /* arp.rs:132 (unreachable)               */
    ZP_ERR_ARP_INVALID_OPER = 7,      /* parser.rs:176                          */
    ZP_ERR_IPV4_TOO_SHORT = 8,        /* ipv4.rs:140 (encapsulated levels only) */
    ZP_ERR_IPV4_VERSION = 9,          /* parser.rs:192                          */
    ZP_ERR_IPV4_IHL_TOO_SHORT = 10,   /* parser.rs:196                          */
    ZP_ERR_IPV4_HDR_TOO_LONG = 11,    /* parser.rs:200                          */
    ZP_ERR_IPV4_TOTAL_LENGTH = 12,    /* parser.rs:204                          */
    ZP_ERR_IPV4_CHECKSUM = 13,        /* parser.rs:208                          */
    ZP_ERR_IPV4_HDR_EXCEEDS = 14,     /* ipv4.rs:240,254 (unreachable)          */
    ZP_ERR_IPV6_TOO_SHORT = 15,       /* ipv6.rs:149 (encapsulated levels only) */
    ZP_ERR_IPV6_VERSION = 16,         /* parser.rs:226                          */
    ZP_ERR_EXT_HBH_NOT_FIRST = 17,    /* headers.rs:99-101                      */
    ZP_ERR_EXT_OPTIONS_TOO_SHORT = 18,/* options.rs:85                          */
    ZP_ERR_EXT_OPTIONS_EXCEEDS = 19,  /* options.rs:149                         */
    ZP_ERR_EXT_ROUTING_TOO_SHORT = 20,/* routing.rs:109                         */
    ZP_ERR_EXT_ROUTING_EXCEEDS = 21,  /* routing.rs:190                         */
    ZP_ERR_EXT_FRAGMENT_TOO_SHORT = 22,/* fragment.rs:99                        */
    ZP_ERR_EXT_AUTH_TOO_SHORT = 23,   /* authentication.rs:107                  */
    ZP_ERR_EXT_AUTH_EXCEEDS = 24,     /* authentication.rs:195                  */
    ZP_ERR_TCP_TOO_SHORT = 25,        /* tcp.rs:143                             */
    ZP_ERR_TCP_DATA_OFFSET = 26,      /* parser.rs:242                          */
    ZP_ERR_TCP_FLAGS = 27,            /* parser.rs:246                          */
    ZP_ERR_UDP_TOO_SHORT = 28,        /* udp.rs:105                             */
    ZP_ERR_UDP_LENGTH = 29,           /* parser.rs:262                          */
    ZP_ERR_ICMP_TOO_SHORT = 30,       /* icmpv4.rs:94 == icmpv6.rs:91           */
    ZP_ERR_ICMPV4_TYPE = 31,          /* parser.rs:278                          */
    ZP_ERR_ICMPV4_CODE = 32,          /* parser.rs:282                          */
    ZP_ERR_ICMPV6_TYPE = 33,          /* parser.rs:298                          */
    ZP_ERR_IPV4_L4_CHECKSUM = 34,     /* parser.rs:329                          */
    ZP_ERR_IPV6_L4_CHECKSUM = 35,     /* parser.rs:357                          */
    /* Errors of the reader accessors only (parse() never returns them):    */
    ZP_ERR_TCP_HDR_EXCEEDS = 36,      /* tcp.rs:227,239 (header()/payload())    */
    ZP_ERR_OPTIONS_DATA_EXCEEDS = 37, /* options.rs:115 (options())             */
    ZP_ERR_COUNT = 38
} zp_err;

/* ------------------------------------------------------------------------- */
/* Presence bits of zp_record.flags: the nine Option fields of PacketParser   */
/* (parser.rs:23-31) plus the IpInIp tag (misc.rs:6-9) and the two            */
/* Option<ExtensionHeaders> (ipv6.rs:140) with their six Option readers each  */
/* (headers.rs:20-25).                                                        */
/* ------------------------------------------------------------------------- */
#define ZP_F_ETHERNET      (1u << 0)
#define ZP_F_ARP           (1u << 1)
#define ZP_F_IPV4          (1u << 2)   /* outermost IPv4 (from Ethernet)        */
#define ZP_F_IPV6          (1u << 3)   /* outermost IPv6 (from Ethernet)        */
#define ZP_F_IP_IN_IP      (1u << 4)   /* first encapsulated IP header          */
#define ZP_F_IP_IN_IP_V6   (1u << 5)   /* ... and it is IpInIp::Ipv6            */
#define ZP_F_TCP           (1u << 6)
#define ZP_F_UDP           (1u << 7)
#define ZP_F_ICMPV4        (1u << 8)
#define ZP_F_ICMPV6        (1u << 9)
#define ZP_F_EXT           (1u << 10)  /* ipv6.extension_headers.is_some()      */
#define ZP_F_INNER_EXT     (1u << 11)  /* ip_in_ip IPv6 extension_headers Some  */
/* Extension header slots, in ExtensionHeaders field order (headers.rs:20-25). */
#define ZP_EXT_HBH   0
#define ZP_EXT_RT    1
#define ZP_EXT_FRAG  2
#define ZP_EXT_AH    3
#define ZP_EXT_DST1  4
#define ZP_EXT_DST2  5
#define ZP_EXT_SLOTS 6
#define ZP_F_EXT_SLOT(k)       (1u << (12 + (k)))  /* outer set, k in [0,6) */
#define ZP_F_INNER_EXT_SLOT(k) (1u << (18 + (k)))  /* inner set             */

/*
 * One parse result, 8 bytes (one dwordx2 store per frame). The record writes
 * are the only HBM writes of the parse, and writes mixed into the read
 * stream cost several times their bytes: the 8-B record took
 * 2-7 % off every configuration against the 16-B record of ABI v2/v3.
 *
 *   flags  bits  0-23  ZP_F_* presence and extension-slot bits (above)
 *          bits 24-25  Ethernet code: header length 14 + 4 * code (14 / 18 /
 *                      22, ethernet.rs:155-179); code 3 = the far-L4 form
 *          bits 26-31  err (zp_err; ZP_OK = 0)
 *   offs   bits  0-17  l4_off: start of the single tcp/udp/icmpv4/icmpv6 reader
 *          bits 18-31  inner_off: start of the ip_in_ip header (always below
 *                      16,384: Ethernet 22 + IPv6 40 + the longest chain 9,228)
 *
 * All offsets are FRAME offsets (bytes from the first byte of the frame).
 * ethernet/arp/ipv4/ipv6 start at offsets 0 / eth_len / eth_len / eth_len.
 * When err != ZP_OK the reference returns Err and no PacketParser exists:
 * the record is then zero except the err bits.
 *
 * Far-L4 form (ABI v5). An L4 reader that starts past ZP_L4_NEAR_MAX
 * (262,143) does not fit 18 bits; only an IPv6 jumbogram with thousands of
 * nested IPv6 headers reaches it (parser.rs:134-135 recurses without limit,
 * ipv6.rs:147-167 never checks payload_length). Its record carries Ethernet
 * code 3 and offs = the whole 32-bit L4 offset. The Ethernet header length
 * and inner_off, which such a frame always has (its first IP level ends by
 * byte 9,290), are then read from the frame, exactly as the parse found them:
 * eth_len by ethernet.rs:155-179, inner_off = eth_len + the outer IP header
 * (IPv4: IHL * 4; IPv6: 40 + extension_headers_len, the outer ext entry's
 * len). zp_rec_decode() does this; the facades call it. Every result stays
 * exact: nothing saturates.
 *
 * IPv6Reader::final_next_header() (ipv6.rs:219-227) is not in the record:
 * for an IPv6 header with an extension chain it is the chain's
 * final_next_header (headers.rs:26), stored in its zp_ext_offsets entry;
 * without a chain it is the header's next-header byte (frame offset ip + 6).
 */
typedef struct zp_record {
    uint32_t flags;
    uint32_t offs;
} zp_record;

#define ZP_F_MASK        0x00FFFFFFu
#define ZP_L4_NEAR_MAX   0x3FFFFu   /* largest l4_off of the ordinary form   */
#define ZP_ETH_CODE_FAR  3u         /* flags bits 24-25 of the far-L4 form   */
static inline uint32_t zp_rec_err(zp_record r)     { return r.flags >> 26; }
static inline int      zp_rec_is_far(zp_record r)  { return ((r.flags >> 24) & 3u) == ZP_ETH_CODE_FAR; }
static inline uint32_t zp_rec_l4_off(zp_record r)  { return zp_rec_is_far(r) ? r.offs : r.offs & ZP_L4_NEAR_MAX; }
/* Ordinary form only (0 for a far-L4 record: zp_rec_decode reads them from the frame). */
static inline uint32_t zp_rec_eth_len(zp_record r)   { return zp_rec_is_far(r) ? 0u : 14u + 4u * ((r.flags >> 24) & 3u); }
static inline uint32_t zp_rec_inner_off(zp_record r) {
    return zp_rec_is_far(r) || !(r.flags & ZP_F_IP_IN_IP) ? 0u : r.offs >> 18;
}

/*
 * Inline outer chain (ABI v6). A frame without an ip_in_ip header leaves the
 * inner_off field (offs bits 18-31) free. When its outer IPv6 extension chain
 * is short and in RFC 8200 order and the frame has an L4 reader, the chain is
 * stored there and its ext entry is NOT written (c4-shaped traffic then
 * writes 8 B per frame instead of 8 + 16):
 *
 *   offs bit 31      ZP_CHAIN_INLINE
 *   offs bits 18-20  Hop-by-Hop  length code c: (c + 1) * 8 B   (options.rs:123)
 *   offs bits 21-22  Destination 1st         c: (c + 1) * 8 B
 *   offs bits 23-25  Routing                 c: (c + 1) * 8 B   (routing.rs:164)
 *   (Fragment: always 8 B, fragment.rs:158)
 *   offs bits 26-27  Authentication          c: (c + 2) * 4 B   (authentication.rs:173)
 *   offs bits 28-29  Destination 2nd         c: (c + 1) * 8 B
 *
 * The present headers (the record's ZP_F_EXT_SLOT bits) lie back to back in
 * the order Hop-by-Hop, Destination 1st, Routing, Fragment, Authentication,
 * Destination 2nd; slot offsets are the running sums, extension_headers_len
 * the total, and final_next_header (headers.rs:26) the protocol of the
 * record's L4 reader (6 / 17 / 1 / 58). zp_rec_chain() rebuilds the
 * zp_ext_offsets entry; the host paths (zp_parse_batch_host, zp_parse_one,
 * the ring) hand out the rebuilt entry, so only device-batch callers see the
 * inline form. Any other chain keeps its 16-B entry.
 */
#define ZP_CHAIN_INLINE (1u << 31)
static inline int zp_rec_chain_inline(zp_record r) {
    return (r.flags >> 26) == 0 && !zp_rec_is_far(r) &&
           (r.flags & (ZP_F_EXT | ZP_F_IP_IN_IP)) == ZP_F_EXT && (r.offs & ZP_CHAIN_INLINE) != 0;
}

/*
 * One IPv6 extension chain (Some(ExtensionHeaders), headers.rs:19-28), 16 B:
 * len = IPv6Reader::extension_headers_len (ipv6.rs:141), off[k] = start of
 * slot k relative to the IPv6 payload (frame offset ip + 40 + off[k]),
 * final_nh = ExtensionHeaders::final_next_header (headers.rs:26).
 *
 * The ext side array of a batch of n frames holds 2n entries:
 *   ext[i]     the outer ipv6 chain of frame i, valid iff flags & ZP_F_EXT and
 *              the chain is not inline (zp_rec_chain_inline; device batches only);
 *   ext[n + i] the ip_in_ip IPv6 chain,           valid iff flags & ZP_F_INNER_EXT.
 * Entries whose flag is clear are unspecified (the kernel may leave them
 * untouched or zero them). Passing ext = NULL drops the chains (the records
 * still carry their presence and slot bits).
 */
typedef struct zp_ext_offsets {
    uint16_t len;
    uint16_t off[ZP_EXT_SLOTS];
    uint8_t  final_nh;
    uint8_t  reserved;
} zp_ext_offsets;

/* The zp_ext_offsets entry of an inline outer chain (zp_rec_chain_inline(r)
 * must hold): slot offsets, extension_headers_len and final_next_header. */
static inline void zp_rec_chain(zp_record r, zp_ext_offsets* x) {
    static const uint8_t order[6] = {ZP_EXT_HBH, ZP_EXT_DST1, ZP_EXT_RT, ZP_EXT_FRAG,
                                     ZP_EXT_AH, ZP_EXT_DST2};
    const uint32_t c = r.offs >> 18;
    const uint32_t len[6] = {                         /* by slot                   */
        ((c & 7u) + 1u) * 8u,                         /* ZP_EXT_HBH,  bits 18-20   */
        (((c >> 5) & 7u) + 1u) * 8u,                  /* ZP_EXT_RT,   bits 23-25   */
        8u,                                           /* ZP_EXT_FRAG               */
        (((c >> 8) & 3u) + 2u) * 4u,                  /* ZP_EXT_AH,   bits 26-27   */
        (((c >> 3) & 3u) + 1u) * 8u,                  /* ZP_EXT_DST1, bits 21-22   */
        (((c >> 10) & 3u) + 1u) * 8u};                /* ZP_EXT_DST2, bits 28-29   */
    uint32_t at = 0;
    for (int k = 0; k < ZP_EXT_SLOTS; ++k) x->off[k] = 0;
    for (int j = 0; j < 6; ++j) {
        const int k = order[j];
        if (r.flags & ZP_F_EXT_SLOT(k)) { x->off[k] = (uint16_t)at; at += len[k]; }
    }
    x->len = (uint16_t)at;
    x->final_nh = (uint8_t)((r.flags & ZP_F_TCP) ? 6 : (r.flags & ZP_F_UDP) ? 17
                          : (r.flags & ZP_F_ICMPV4) ? 1 : 58);
    x->reserved = 0;
}

/* A record with every field unpacked (PacketParser's readers by start
 * offset): flags = ZP_F_* bits, eth_len 14/18/22, final_nh / inner_final_nh
 * = IPv6Reader::final_next_header() (ipv6.rs:219-227) of the outer /
 * ip_in_ip IPv6 header (0 where absent); all zero but err on an error. */
typedef struct zp_rec_fields {
    uint32_t flags;
    uint8_t  err, eth_len, final_nh, inner_final_nh;
    uint32_t inner_off, l4_off;
} zp_rec_fields;

/* Unpacks `*rec`, the record of `frame` (len bytes), both forms (see above).
 * ext: NULL or the frame's two entries (outer chain, ip_in_ip chain); where
 * the record flags a chain and ext is NULL the chain is re-walked over the
 * frame (ipv6.rs:147-167), which gives the same values for a frame the
 * parse accepted. Host code. Returns 0, or -1 when the record cannot belong
 * to this frame (an offset past its end, a far record without an L4 reader
 * or an ip_in_ip header). */
int zp_rec_decode(const zp_record* rec, const uint8_t* frame, uint64_t len,
                  const zp_ext_offsets* ext, zp_rec_fields* out);

/* ------------------------------------------------------------------------- */
/* Library info                                                              */
/* ------------------------------------------------------------------------- */
/* Returns ZP_ABI_VERSION. */
int zp_abi_version(void);
/* Exact reference error string for a zp_err code ("" for ZP_OK, NULL if out
 * of range). Replaces the `&'static str` of Result (parser.rs:53). */
const char* zp_err_str(int code);
/* Last HIP error string seen by this library on the calling thread. */
const char* zp_last_error(void);

/* ------------------------------------------------------------------------- */
/* Batch parse — the hot path.                                                */
/* Replaces a loop of PacketParser::parse(&arena[off[i]..off[i]+len[i]])      */
/* (parser.rs:53) over n frames.                                              */
/* ------------------------------------------------------------------------- */
/*
 * Device-resident batch parse. All pointers are device memory on the current
 * HIP device; the call only enqueues work on `stream` (a hipStream_t, NULL =
 * default stream) and returns. Frames may lie anywhere in `arena` (gaps,
 * overlaps and any order are allowed); the fast path is taken for the common
 * packed, increasing layout. `ext` (2n entries, see zp_ext_offsets) may be
 * NULL. Returns 0 on success or
 * a negative value if the launch failed (see zp_last_error()).
 * Precondition (not checked on the device: the descriptors live in HBM and the
 * call does not synchronise): offs[i] + lens[i] <= the arena's size for every
 * i. A descriptor past the arena reads past the allocation and faults the
 * GPU. The Python wrapper (batch.parse_batch) checks this with one device
 * reduction unless told not to.
 */
int zp_parse_batch_device(const uint8_t* arena, const uint64_t* offs,
                          const uint32_t* lens, uint64_t n,
                          zp_record* records, zp_ext_offsets* ext,
                          void* stream);

/*
 * Record codes (round 6). Inside the parse's read stream a record store
 * costs in proportion to the contiguous bytes a wave stores,
 * so a full tile of 64 frames whose records all have the common form (no
 * error, no IP-in-IP, no extension headers, the L4 reader right after a
 * 20-B IPv4 or 40-B IPv6 header: config 3) is stored as one code byte per
 * frame over the tile's first 8 records, and a second kernel on the same
 * stream rewrites the tile's 64 records from the codes. The records a
 * caller reads are the same either way (zp_parse_batch_device still only
 * enqueues). mode 0: automatic (batches of at least 2,097,152 frames
 * whose traffic has code tiles: probe calls, one per 16 calls per device
 * and one at every change of batch size, tell, through a mapped host word
 * their second kernel sets and an event queried without waiting), 1:
 * always, 2: never. Process-wide; returns the previous mode, or -1 for an
 * unknown mode.
 */
int zp_set_record_slots(int mode);
/* The automatic mode's current decision on the calling thread's device for
 * batches of at least 2,097,152 frames (1: record codes, 0: one kernel);
 * the latest completed probe's verdict, 1 before any. For reports. */
int zp_record_slots_state(void);

/* Host-buffer convenience path: the frames, descriptors and outputs live in
 * host memory (a NIC ring / raw socket buffer). Stages through pinned buffers
 * and overlaps H2D copy, parse and D2H copy in chunks on `ctx`'s streams.
 * Synchronous. Returns 0 on success, negative on HIP failure.
 * A zp_ctx owns pinned staging buffers, device buffers and streams: it must
 * not be used by two host threads at once (one context per thread, or a
 * lock around every call that takes it, as the Python facade does). */
typedef struct zp_ctx zp_ctx;
zp_ctx* zp_ctx_create(int device, uint64_t chunk_bytes);
void    zp_ctx_destroy(zp_ctx* ctx);
int zp_parse_batch_host(zp_ctx* ctx, const uint8_t* arena, uint64_t arena_bytes,
                        const uint64_t* offs, const uint32_t* lens, uint64_t n,
                        zp_record* records, zp_ext_offsets* ext);
/* The same over several devices (one context each, e.g. the 8 GPUs of a
 * node): contiguous frame ranges with balanced byte totals run concurrently,
 * one host thread per context. No cross-device exchange. Returns 0 or the
 * first failing context's code (zp_last_error() names the context). */
int zp_parse_batch_host_multi(zp_ctx* const* ctxs, int nctx, const uint8_t* arena,
                              uint64_t arena_bytes, const uint64_t* offs,
                              const uint32_t* lens, uint64_t n, zp_record* records,
                              zp_ext_offsets* ext);
/* One frame through the GPU path (PacketParser::parse equivalent,
 * parser.rs:53). ext: NULL or 2 entries (outer, ip_in_ip chain; zeroed where
 * the record flags no chain). Returns the zp_err code (>= 0) or a negative
 * value on HIP failure. The frame is copied into ctx's mapped pinned block;
 * by default the device's shared resident server (one kernel per device and
 * process, one wave per context, launched on demand) polls a doorbell there,
 * parses the frame in place and writes the record back: no kernel launch per
 * call. The kernel leaves after 1 ms resident whatever
 * the traffic; the next call replaces it (under steady traffic a caller
 * queues the next one and retires the old one). A device-wide
 * synchronisation (hipDeviceSynchronize, torch.cuda.synchronize, hipFree)
 * issued meanwhile waits for the running kernel, so about 1 ms at most;
 * zp_parse_one_config stops it at once. Frames over 64 KiB take the batch
 * host path. Like every zp_ctx call, one thread at a time per ctx (one
 * context per thread, or a pool); contexts of one device share the server,
 * so their calls run concurrently. */
int zp_parse_one(zp_ctx* ctx, const uint8_t* frame, uint64_t len,
                 zp_record* record, zp_ext_offsets ext[2]);
/* zp_parse_one's mode on ctx: idle_us > 0 = the device's resident server
 * (the default, 5000; the value is no longer a timeout: the server's life is
 * 1 ms); 0 = one batch-kernel launch and a stream wait per call (~18 us).
 * Stops the device's server either way (every context's next call
 * relaunches it). Returns 0, or -1 on a NULL ctx. */
int zp_parse_one_config(zp_ctx* ctx, uint32_t idle_us);
/* The calling thread's current HIP device (hipGetDevice), -1 on failure:
 * the device a facade creates its contexts on. */
int zp_device_current(void);

/* ------------------------------------------------------------------------- */
/* Standalone readers and the checksum primitives.                           */
/* The reference's second usage (README.md:110-115) builds a reader directly */
/* over a slice: TcpReader::new(&packet[off..])? and reads its fields. Every  */
/* reader's `new` is a checked constructor returning Result (the minimum     */
/* slice length; Ethernet also the VLAN tagging; IPv6 also the extension    */
/* walk, ipv6.rs:159). These are host-side views over host bytes, like the  */
/* reference's: one slice, no batch, no device. The batch parse stays the   */
/* device path above.                                                        */
/* ------------------------------------------------------------------------- */
typedef enum zp_reader_kind {
    ZP_READER_ETHERNET = 0,  /* EthernetReader::new               ethernet.rs:141 */
    ZP_READER_ARP = 1,       /* ArpReader::new                    arp.rs:130      */
    ZP_READER_IPV4 = 2,      /* IPv4Reader::new                   ipv4.rs:138     */
    ZP_READER_IPV6 = 3,      /* IPv6Reader::new (+ extension walk) ipv6.rs:147-167 */
    ZP_READER_OPTIONS = 4,   /* OptionsHeaderReader::new          options.rs:83   */
    ZP_READER_ROUTING = 5,   /* RoutingHeaderReader::new          routing.rs:107  */
    ZP_READER_FRAGMENT = 6,  /* FragmentHeaderReader::new         fragment.rs:97  */
    ZP_READER_AUTH = 7,      /* AuthenticationHeaderReader::new   authentication.rs:105 */
    ZP_READER_TCP = 8,       /* TcpReader::new                    tcp.rs:141      */
    ZP_READER_UDP = 9,       /* UdpReader::new                    udp.rs:103      */
    ZP_READER_ICMPV4 = 10,   /* Icmpv4Reader::new                 icmpv4.rs:92    */
    ZP_READER_ICMPV6 = 11,   /* Icmpv6Reader::new                 icmpv6.rs:89    */
    ZP_READER_KIND_COUNT = 12
} zp_reader_kind;

/* What a successful constructor computed besides the slice itself. */
typedef struct zp_reader_info {
    uint32_t header_len;     /* Ethernet: 14/18/22 (calculate_header_len,      */
                             /* ethernet.rs:155-179); 0 for the other kinds    */
    uint32_t flags;          /* IPv6: ZP_F_EXT when extension_headers is Some, */
                             /* ZP_F_EXT_SLOT(k) per present slot; else 0      */
    uint8_t  final_nh;       /* IPv6: final_next_header() (ipv6.rs:219-227)    */
    uint8_t  reserved[3];
    zp_ext_offsets ext;      /* IPv6: extension_headers_len (ext.len) and the  */
                             /* slot offsets, relative to the IPv6 payload     */
} zp_reader_info;

/* XReader::new(&bytes[..len]) of reader `kind`. Returns ZP_OK (info filled,
 * when not NULL) or the zp_err code of the reference's Err, whose string is
 * zp_err_str(code); -1 for an unknown kind or bytes == NULL with len > 0. */
int zp_reader_new(int kind, const uint8_t* bytes, uint64_t len, zp_reader_info* info);

/* internet_checksum(data, accumulator) (checksum.rs:5-29): RFC 1071 sum of
 * the big-endian 16-bit words (an odd tail byte as the high byte) with u32
 * wrap-around, folded, complemented. */
uint16_t zp_internet_checksum(const uint8_t* data, uint64_t len, uint32_t accumulator);
/* verify_internet_checksum (checksum.rs:33-35): 1 if the checksum is 0. */
int zp_verify_internet_checksum(const uint8_t* data, uint64_t len, uint32_t accumulator);
/* pseudo_header(src, dest, protocol, length) (checksum.rs:38-69) for 4-byte
 * (IPv4) or 16-byte (IPv6) addresses: the address words + protocol +
 * (u32)length. addr_len other than 4 or 16 returns 0. */
uint32_t zp_pseudo_header(const uint8_t* src, const uint8_t* dest, uint32_t addr_len,
                          uint8_t protocol, uint64_t length);

/* ------------------------------------------------------------------------- */
/* Per-batch counters: frames per presence bit of          */
/* zp_record.flags and frames per zp_err code, for monitoring a capture      */
/* (protocol mix, error histogram) without copying the records to the host. */
/* ------------------------------------------------------------------------- */
#define ZP_STATS_FLAG_BITS 24                      /* flags bits 0-23 (ZP_F_*, slots) */
#define ZP_STAT_FLAG(bit)  (bit)                   /* frames with flags bit `bit` set */
#define ZP_STAT_ERR(code)  (ZP_STATS_FLAG_BITS + (code))  /* frames with err == code   */
#define ZP_STATS_COUNT     (ZP_STATS_FLAG_BITS + ZP_ERR_COUNT)
/* Adds the counts of records[0, n) into counts[ZP_STATS_COUNT] (device u64,
 * zeroed by the caller; several batches accumulate). Enqueues on `stream`.
 * The counts of several devices add up on the host (frames are independent).
 * Returns 0 or negative on launch failure. */
int zp_stats_device(const zp_record* records, uint64_t n, uint64_t* counts, void* stream);

/* Diagnostic: one plain streaming read of bytes [p, p + bytes) (device
 * memory, 16-B aligned; the tail below 16 B is not read), enqueued on
 * `stream`. bench.py times it over the arena beside the parse: the parse's
 * rate moves with the physical placement of the arena and so
 * does a pure read, which tells placements apart. sink: one device u32
 * (practically never written). Returns 0 or negative. */
int zp_probe_read_device(const uint8_t* p, uint64_t bytes, uint32_t* sink, void* stream);
/* Diagnostic: the parse kernel's memory traffic without its work. Over
 * ceil(n / 64) waves (one per workgroup, with a parse wave's LDS, so at its
 * occupancy) wave t loads descriptors offs / lens [64 t, 64 t + 64) ∩ [0, n)
 * (when both are given), streams the t-th equal slice of [p, p + bytes) and
 * then, when records != NULL, stores the 8-B words records[64 t, 64 t + 64)
 * ∩ [0, n) (their contents are junk), as the parse does per tile. bench.py
 * times it over the bench's own arena, descriptors and records
 * (roofline.placement). Returns 0 or negative. */
int zp_probe_tiles_device(const uint8_t* p, uint64_t bytes, uint64_t n, const uint64_t* offs,
                          const uint32_t* lens, zp_record* records, uint32_t* sink,
                          void* stream);
/* Diagnostic: the same pattern with record codes (zp_set_record_slots): a
 * full tile stores one byte per frame instead of its 8-B records and the
 * parse's expansion kernel then rewrites records [0, n) (junk contents). */
int zp_probe_tiles_codes_device(const uint8_t* p, uint64_t bytes, uint64_t n,
                                const uint64_t* offs, const uint32_t* lens, zp_record* records,
                                uint32_t* sink, void* stream);

/* ------------------------------------------------------------------------- */
/* Host-ring ingestion pipeline. Frames start in host */
/* memory (a NIC ring / raw socket, README.md:85-115 of the reference). A     */
/* ring holds `nslots` slots, each with pinned host buffers, device buffers   */
/* and its own stream. The producer acquires a slot, fills its arena and      */
/* descriptors in place (a NIC would DMA straight into the pinned arena) and  */
/* submits it; the slot then runs H2D -> parse -> D2H asynchronously while    */
/* the next slot fills. The consumer takes completed slots in submission      */
/* order (wait / poll), reads the records and releases the slot.              */
/* Slot states: FREE -acquire-> FILLING -submit-> IN_FLIGHT -wait/poll->      */
/* DONE -release-> FREE. One producer and one consumer thread may use a ring  */
/* concurrently. All functions return 0 on success, negative on error (see    */
/* zp_last_error()), ZP_RING_TIMEOUT when a wait expires.                     */
/* ------------------------------------------------------------------------- */
typedef struct zp_ring zp_ring;
#define ZP_RING_TIMEOUT (-4)
typedef struct zp_ring_slot {
    int32_t id;                         /* slot index                          */
    uint8_t* arena;                     /* pinned host arena, arena_cap bytes  */
    uint64_t* offs;                     /* pinned frame offsets into arena     */
    uint32_t* lens;                     /* pinned frame lengths                */
    uint64_t arena_cap, frames_cap;
    const zp_record* records;           /* results (valid after wait/poll)     */
    const zp_ext_offsets* ext;          /* 2n entries (zp_ext_offsets), n below */
    uint64_t n;                         /* frames in the slot (after wait/poll) */
    uint64_t seq;                       /* submission sequence number          */
} zp_ring_slot;

zp_ring* zp_ring_create(int device, uint32_t nslots, uint64_t slot_bytes,
                        uint64_t slot_frames);
void zp_ring_destroy(zp_ring* ring);
/* Hands out the next slot (in ring order) once it is FREE, as FILLING.
 * timeout_ms < 0 blocks, 0 only checks; ZP_RING_TIMEOUT when it expires. */
int zp_ring_acquire(zp_ring* ring, zp_ring_slot* slot, int64_t timeout_ms);
/* Enqueues H2D + parse + D2H for the first n frames of an acquired slot.
 * Frames must lie inside the slot arena (else -1, nothing enqueued). */
int zp_ring_submit(zp_ring* ring, int32_t id, uint64_t n);
/* Hands out the oldest submitted slot once its records are in host memory.
 * timeout_ms < 0 blocks, 0 polls; ZP_RING_TIMEOUT when nothing is ready. */
int zp_ring_wait(zp_ring* ring, zp_ring_slot* slot, int64_t timeout_ms);
/* Returns a DONE slot to the producer. */
int zp_ring_release(zp_ring* ring, int32_t id);

/* ------------------------------------------------------------------------- */
/* Column views: the reader getters of every parsed  */
/* frame gathered into SoA device columns, so downstream consumers get ready */
/* columns (5-tuple, VLAN TCIs, flow label ...) without a host pass.         */
/* Entry i of a column is 0 when record i holds an error or the reader the   */
/* column belongs to is absent. Multi-byte integers are host order (LE);     */
/* byte-array columns (MACs, addresses) are the frame bytes as they stand.   */
/* "outer IP" = PacketParser::ipv4 / ::ipv6, "inner IP" = ::ip_in_ip.        */
/* ------------------------------------------------------------------------- */
typedef enum zp_col {
    ZP_COL_DEST_MAC = 0,     /* u8[6]  EthernetReader::dest_mac (ethernet.rs:195-198)     */
    ZP_COL_SRC_MAC,          /* u8[6]  EthernetReader::src_mac (ethernet.rs:201-204)      */
    ZP_COL_ETHERTYPE,        /* u16    EthernetReader::ethertype (ethernet.rs:209-212)    */
    ZP_COL_VLAN_TCI,         /* u16    vlan_tag().1, or double_vlan_tag().0.1 (:218-244)  */
    ZP_COL_VLAN_INNER_TCI,   /* u16    double_vlan_tag().1.1 (ethernet.rs:232-244)        */
    ZP_COL_ARP_OPER,         /* u16    ArpReader::oper (arp.rs:174-177)                   */
    ZP_COL_IP_VERSION,       /* u8     4 or 6 when the outer IP reader is present         */
    ZP_COL_SRC_ADDR,         /* u8[16] IPv4Reader::src_ip in bytes 0-3 (ipv4.rs:210-213)  */
                             /*        or IPv6Reader::src_addr (ipv6.rs:245-248)          */
    ZP_COL_DEST_ADDR,        /* u8[16] dest_ip (ipv4.rs:216-219) / dest_addr (ipv6.rs:253-256) */
    ZP_COL_PROTOCOL,         /* u8     IPv4 protocol (ipv4.rs:204-207) / IPv6             */
                             /*        final_next_header (ipv6.rs:219-227)                */
    ZP_COL_TTL,              /* u8     ttl (ipv4.rs:198-201) / hop_limit (ipv6.rs:237-240) */
    ZP_COL_TOS,              /* u8     dscp<<2|ecn (ipv4.rs:160-169) / traffic_class (ipv6.rs:181) */
    ZP_COL_IP_ID,            /* u32    IPv4 id (ipv4.rs:180) / flow_label (ipv6.rs:189)    */
    ZP_COL_IP_LEN,           /* u16    total_length (ipv4.rs:174) / payload_length (ipv6.rs:199)*/
    ZP_COL_INNER_VERSION,    /* u8     4 or 6 when ip_in_ip is present (misc.rs:6-9)      */
    ZP_COL_INNER_SRC_ADDR,   /* u8[16] as ZP_COL_SRC_ADDR, of the ip_in_ip reader         */
    ZP_COL_INNER_DEST_ADDR,  /* u8[16]                                                    */
    ZP_COL_INNER_PROTOCOL,   /* u8     protocol / final_next_header of ip_in_ip           */
    ZP_COL_L4_PROTO,         /* u8     6 tcp, 17 udp, 1 icmpv4, 58 icmpv6; 0 none         */
    ZP_COL_SRC_PORT,         /* u16    TcpReader / UdpReader::src_port (tcp.rs:151, udp.rs:113) */
    ZP_COL_DEST_PORT,        /* u16    dest_port (tcp.rs:157, udp.rs:119)                 */
    ZP_COL_TCP_SEQ,          /* u32    sequence_number (tcp.rs:163-170)                   */
    ZP_COL_TCP_ACK,          /* u32    ack_number (tcp.rs:172-179)                        */
    ZP_COL_TCP_FLAGS,        /* u8     flags (tcp.rs:193-196)                             */
    ZP_COL_TCP_WINDOW,       /* u16    window_size (tcp.rs:199-202)                       */
    ZP_COL_ICMP_TYPE,        /* u8     icmp_type (icmpv4.rs:102, icmpv6.rs:99)            */
    ZP_COL_ICMP_CODE,        /* u8     icmp_code (icmpv4.rs:108, icmpv6.rs:105)           */
    ZP_COL_L4_CHECKSUM,      /* u16    checksum() (tcp.rs:205, udp.rs:125, icmpv4.rs:114) */
    ZP_COL_PAYLOAD_OFF,      /* u32    frame offset of the L4 reader's payload(); 0 when  */
                             /*        absent or when payload() returns Err (tcp.rs:235-243) */
    ZP_COL_COUNT
} zp_col;

/* Element size in bytes of column `col` (0 if out of range). */
int zp_col_width(int col);

/* Fills the requested columns for n parsed frames: cols[c] is a device array
 * of n * zp_col_width(c) bytes, or NULL to skip column c. arena/offs/lens are
 * the batch given to zp_parse_batch_device, records its output (device
 * memory). Enqueues on `stream`; returns 0 or negative on launch failure. */
int zp_extract_columns_device(const uint8_t* arena, const uint64_t* offs,
                              const uint32_t* lens, const zp_record* records, uint64_t n,
                              void* const* cols, void* stream);

/* zp_parse_batch_device and zp_extract_columns_device fused: one pass over
 * the frames writes the records and the requested columns (read from the
 * parse kernel's staged header window; cols as above, NULL entries skipped).
 * Same results as the two calls in sequence. */
int zp_parse_batch_columns_device(const uint8_t* arena, const uint64_t* offs,
                                  const uint32_t* lens, uint64_t n, zp_record* records,
                                  zp_ext_offsets* ext, void* const* cols, void* stream);

/* ------------------------------------------------------------------------- */
/* Batched header rewrite: the writers' field setters over frames that exist  */
/* already (EthernetWriter::set_src_mac, IPv4Writer::set_ttl / set_src_ip,    */
/* IPv6Writer::set_hop_limit, TcpWriter::set_src_port ...), with the          */
/* checksums refreshed. The inverse of the column views: extract, edit the    */
/* columns, write them back (NAT, TTL decrement, DSCP re-marking, VLAN        */
/* re-tagging, MAC rewrite) without a host pass and without touching the      */
/* payload.                                                                   */
/*                                                                            */
/* Writable columns: DEST_MAC, SRC_MAC (the MAC bytes), VLAN_TCI,             */
/* VLAN_INNER_TCI (the TCI only; the TPIDs stay), SRC_ADDR, DEST_ADDR (outer  */
/* IP), TTL (ttl / hop limit), TOS (IPv4 byte 1 whole / IPv6 traffic class),  */
/* IP_ID (IPv4 id from the low 16 bits / IPv6 flow label from the low 20),    */
/* SRC_PORT, DEST_PORT (TCP or UDP), TCP_SEQ, TCP_ACK, TCP_WINDOW.            */
/*                                                                            */
/* 1. A frame whose record holds an error or no Ethernet reader is left       */
/*    byte for byte as it is.                                                 */
/* 2. Entry i of a column applies to frame i exactly when the extract of that */
/*    column would read a present reader (TCP_* with a TCP reader, ports with */
/*    TCP or UDP, the IP columns with an outer IPv4 / IPv6 reader, VLAN_TCI   */
/*    with one or two tags, VLAN_INNER_TCI with two); other entries are       */
/*    ignored.                                                                */
/* 3. Afterwards the frame is what the writers give: the setters of the       */
/*    applied fields, then IPv4Writer::set_checksum (ipv4.rs:119-126) under   */
/*    an outer IPv4, then the L4 writer's set_checksum(pseudo_sum) over the   */
/*    L4 slice to the frame end (tcp.rs:123-129, udp.rs:65-71,                */
/*    icmpv4.rs:74-80, icmpv6.rs:71-77). A checksum none of whose covered     */
/*    words (pseudo-header included) got another value is not written, so     */
/*    rewrite(extract(x)) is the identity even over a valid checksum stored   */
/*    as 0xFFFF where a recompute stores 0x0000.                              */
/* 4. The L4 checksum covers the outer addresses as parser.rs:311-362 has it: */
/*    only without ip_in_ip, and not for ICMPv4 under an outer IPv4.          */
/* 5. Nothing else changes: lengths, offsets and presence stay, so the        */
/*    batch's records hold for the rewritten frames.                          */
/* The checksums are updated from the changed words (RFC 1624), which equals  */
/* the recompute because the parse verified them: the frames must be          */
/* unchanged since that parse. The payload is not read, with one exception:   */
/* the reference sums into a u32 that wraps (checksum.rs:5-29), and a sum     */
/* that can reach 2^32 is no longer a sum mod 65535. For a frame whose L4     */
/* slice has ZP_REWRITE_EXACT_L4_BYTES or more (IPv6 jumbograms with TCP or   */
/* ICMP) and whose L4 checksum changes, the new L4 slice is summed in full    */
/* with that wrap, as the L4 writers do.                                      */
/* ------------------------------------------------------------------------- */

/* The shortest L4 slice (frame length - L4 offset) whose word sum plus        */
/* pseudo-header can reach 2^32: below it, with L the slice's length,          */
/* ceil(L / 2) * 0xFFFF (its words, the checksum field included)               */
/* + 16 * 0xFFFF (two IPv6 addresses) + 255 (protocol) + L (length) < 2^32,    */
/* so the reference's sum never wraps and the update from the changed words   */
/* is exact. The bound grows with L; it holds at 131,036 and fails at 131,037. */
#define ZP_REWRITE_EXACT_L4_BYTES 131037u
#define ZP_REWRITE_SUM_BOUND(L) \
    (((L) + 1ull) / 2 * 0xFFFFull + 16 * 0xFFFFull + 255ull + (L))
#if defined(__cplusplus)
static_assert(ZP_REWRITE_SUM_BOUND(ZP_REWRITE_EXACT_L4_BYTES - 1ull) < (1ull << 32) &&
              ZP_REWRITE_SUM_BOUND(ZP_REWRITE_EXACT_L4_BYTES + 0ull) >= (1ull << 32),
              "ZP_REWRITE_EXACT_L4_BYTES is the first length at which the L4 sum can wrap");
#else
_Static_assert(ZP_REWRITE_SUM_BOUND(ZP_REWRITE_EXACT_L4_BYTES - 1ull) < (1ull << 32) &&
               ZP_REWRITE_SUM_BOUND(ZP_REWRITE_EXACT_L4_BYTES + 0ull) >= (1ull << 32),
               "ZP_REWRITE_EXACT_L4_BYTES is the first length at which the L4 sum can wrap");
#endif

/* 1 if column `col` can be written back by zp_rewrite_columns_device, else 0. */
int zp_col_writable(int col);

/* The writers' setters over n parsed frames, in place. cols is indexed by
 * zp_col exactly as for zp_extract_columns_device (same element widths, same
 * byte order, same 16-B address layout with IPv4 in bytes 0-3); NULL = leave
 * that field alone. arena/offs/lens/records are the batch and the records the
 * parse wrote for it; the frames must not have changed since that parse and
 * must not overlap. Device memory; enqueues on `stream`. A non-NULL pointer
 * for a column that is not writable returns a negative value before anything
 * is launched (zp_last_error names the column). */
int zp_rewrite_columns_device(uint8_t* arena, const uint64_t* offs,
                              const uint32_t* lens, const zp_record* records,
                              uint64_t n, const void* const* cols, void* stream);

/* ------------------------------------------------------------------------- */
/* Select and gather: choose parsed frames on the device and hand them on as  */
/* a sub-batch. A record holds frame-relative offsets, so a selected frame's  */
/* record stays valid wherever the frame is copied: a sub-batch is the        */
/* gathered descriptors, records and ext entries, over the same arena (a      */
/* view) or over a freshly packed one, and every entry point above takes it.  */
/*                                                                            */
/* Frame i is selected when all of these hold:                                */
/*   the record predicate over f = record flags & ZP_F_MASK and the record's  */
/*     err: (f & flags_all) == flags_all, (f & flags_none) == 0, flags_any    */
/*     == 0 or (f & flags_any) != 0, and err as ZP_SEL_ERR_* / a zp_err code  */
/*     says (an error record has f == 0);                                     */
/*   min_len <= lens[i] <= max_len;                                           */
/*   every term. A term's value v is exactly the entry i that                 */
/*     zp_extract_columns_device would store for its column: 0 for an error   */
/*     record or an absent reader, an IPv4 address in bytes 0-3 with zeros    */
/*     behind. So a selector that must tell 10.0.0.0/8 from an IPv6 address   */
/*     whose first byte is 0x0A adds a term on ZP_COL_IP_VERSION.             */
/* Terms are ANDed; callers who need OR run two selections and OR the masks.  */
/* ------------------------------------------------------------------------- */
#define ZP_SELECT_MAX_TERMS 8
typedef enum zp_sel_op {
    ZP_SEL_MASK_EQ = 0,   /* (v & b) == a, byte-wise over the column's width          */
    ZP_SEL_MASK_NE = 1,   /* its negation                                             */
    ZP_SEL_RANGE   = 2,   /* a <= v <= b, unsigned; scalar columns (width 1, 2, 4)    */
    ZP_SEL_NOT_RANGE = 3
} zp_sel_op;
typedef struct zp_select_term {      /* 40 bytes */
    uint8_t col;                     /* zp_col                                        */
    uint8_t op;                      /* zp_sel_op                                     */
    uint8_t pad[6];                  /* must be 0                                     */
    uint8_t a[16], b[16];            /* in the column's own layout: LE scalars in the */
} zp_select_term;                    /* first width bytes, byte arrays as extracted   */
#define ZP_SEL_ERR_ANY     (-1)      /* err not looked at                             */
#define ZP_SEL_ERR_NONZERO (-2)      /* any rejected frame                            */
typedef struct zp_select {
    uint32_t flags_all, flags_any, flags_none;  /* over record flags & ZP_F_MASK; flags_any 0 = ignored */
    int32_t  err;                    /* ZP_SEL_ERR_* or a zp_err code (0 = accepted)  */
    uint32_t min_len, max_len;       /* on lens[i], inclusive; 0 / UINT32_MAX = none  */
    uint32_t nterms;
    zp_select_term terms[ZP_SELECT_MAX_TERMS];   /* all must hold (AND)               */
} zp_select;

/* Frames one workgroup of the scan phase covers; a larger batch takes a
 * second scan launch (tests cross this size). */
#define ZP_SELECT_SCAN_FRAMES 262144u

/* Bytes of device scratch zp_select_device needs for n frames. */
uint64_t zp_select_scratch_bytes(uint64_t n);

/* Marks the selected frames of a parsed batch and compacts them, stably (in
 * ascending frame order). `sel` is host memory, everything else device
 * memory. With c frames selected:
 *   mask         optional, ceil(n / 64) words: bit i % 64 of word i / 64 is
 *                frame i's verdict; bits at and past n are 0;
 *   idx          optional, capacity n: idx[0, c) = the selected indices;
 *   packed_offs  optional, capacity n: packed_offs[j] = the sum of lens of the
 *                selected frames before the j-th (the back-to-back layout);
 *   count        required, 2 words: {c, sum of the selected frames' lens}.
 * Entries of idx / packed_offs at and past c are not written. With nterms ==
 * 0 the frames are not read and arena / offs may be NULL; lens may then be
 * NULL too when no length bound is set and packed_offs is NULL (count[1] is
 * then 0). Refused with a negative value before anything is launched
 * (zp_last_error names the cause): a null sel, count, records or scratch,
 * nterms > ZP_SELECT_MAX_TERMS, a term with a column out of range, a nonzero
 * pad, an unknown op or RANGE / NOT_RANGE on a byte-array column, terms
 * without arena / offs / lens, n >= 2^32 with idx, scratch_bytes below
 * zp_select_scratch_bytes(n). n == 0 writes count = {0, 0} and returns 0.
 * Three kernel launches on `stream` (mark, scan, scatter; the scatter only
 * when idx or packed_offs is given): nothing is allocated and nothing waits,
 * so the call captures into a graph. */
int zp_select_device(const uint8_t* arena, const uint64_t* offs, const uint32_t* lens,
                     const zp_record* records, uint64_t n, const zp_select* sel /* host */,
                     uint64_t* mask,        /* optional: ceil(n/64) words, bit i%64 of word i/64 */
                     uint32_t* idx,         /* optional: n entries capacity                      */
                     uint64_t* packed_offs, /* optional: n entries capacity                      */
                     uint64_t* count,       /* required: 2 device words {selected, sum of lens}  */
                     void* scratch, uint64_t scratch_bytes, void* stream);

/* Gathers the first min(m, *count) entries of idx into a sub-batch (m: the
 * host's bound, it sizes the grid; count == NULL: m). Entry j is frame idx[j]:
 *   out_lens[j], out_records[j], out_ext[j] / out_ext[m + j]: element gathers
 *   (each optional; an ext entry is copied whether or not its record flags a
 *   chain);
 *   dst == NULL: out_offs[j] = offs[idx[j]], a view over the same arena;
 *   dst: the frame's lens bytes go to dst + packed_offs[j] and out_offs[j] =
 *   packed_offs[j]. packed_offs is what zp_select_device wrote (ascending,
 *   back to back). Exactly the frames' bytes are written, nothing between or
 *   around them and nothing outside [dst, dst + dst_bytes): a frame that does
 *   not fit is not copied. dst must not overlap the arena. dst_bytes / m,
 *   the average frame dst was sized for, also picks how many entries a
 *   workgroup takes; it changes speed only.
 * Source reads stay inside the 16-B chunks that hold a frame's bytes, as the
 * parse's do. One launch on `stream`; enqueue-only. */
int zp_gather_frames_device(const uint8_t* arena, const uint64_t* offs, const uint32_t* lens,
                            const zp_record* records, const zp_ext_offsets* ext /* opt, 2n */,
                            uint64_t n, const uint32_t* idx, const uint64_t* packed_offs,
                            uint64_t m, const uint64_t* count /* optional device word */,
                            uint8_t* dst /* NULL: a view, no frame is copied */, uint64_t dst_bytes,
                            uint64_t* out_offs, uint32_t* out_lens, zp_record* out_records,
                            zp_ext_offsets* out_ext /* opt, 2m: [j] outer, [m + j] inner */,
                            void* stream);

/* ------------------------------------------------------------------------- */
/* Classify: a first-match rule table over parsed frames. A rule is exactly a */
/* zp_select: frame i matches rule r exactly when zp_select_device with       */
/* rules[r] would select it (the all-zero value of a column whose reader is   */
/* absent or whose record holds an error included). A table holds nrules      */
/* rules in priority order, 1 <= nrules <= ZP_CLASSIFY_MAX_RULES:             */
/*   rule_of[i]  the smallest r whose rule matches frame i, or ZP_RULE_NONE;  */
/*   hits        nrules + 1 entries: frame i ADDS 1 and lens[i] to entry      */
/*               rule_of[i], an unmatched frame to entry nrules. The call     */
/*               adds to what hits holds (the caller zeroes it once), so the  */
/*               counters persist across batches and graph replays; integer   */
/*               adds make them independent of the execution order;           */
/*   mask        the words zp_select_device writes (bit i % 64 of word i /    */
/*               64, bits at and past n zero): frame i's bit is set when bit  */
/*               rule_of[i] of `accept` is set, bit nrules standing for "no   */
/*               rule". accept: a host bitmap of nrules + 1 bits in           */
/*               ceil((nrules + 1) / 64) words; NULL = "matched any rule".    */
/*               zp_flow_aggregate_device / zp_flow_update_device take it.    */
/* ------------------------------------------------------------------------- */
#define ZP_CLASSIFY_MAX_RULES 256
#define ZP_RULE_NONE 0xFFFFFFFFu
typedef struct zp_rule_hits { uint64_t packets, bytes; } zp_rule_hits;

/* Bytes of the compiled form of an nrules table (non-decreasing in nrules; 0
 * for an nrules out of range). */
uint64_t zp_classify_table_bytes(uint32_t nrules);

/* Compiles rules[0, nrules) into `table` (host memory, 4-byte aligned,
 * table_bytes >= zp_classify_table_bytes(nrules)): a private, versioned form
 * the caller copies to the device as it is; the library allocates no device
 * memory and this call touches no device. Identical terms and identical
 * record predicates of different rules are stored once. The same rules give
 * the same zp_classify_table_bytes(nrules) bytes (padding is zero), so tables
 * can be compared and cached.
 * Returns 1 when some rule has terms (the table reads frames), 0 when none
 * has (a record-only table): this is how the host learns what it has to pass
 * to zp_classify_device, which cannot see the device copy.
 * Refused with a negative value, `table` untouched and zp_last_error naming
 * the rule index and the cause: everything zp_select_device refuses of a
 * selector (nterms > ZP_SELECT_MAX_TERMS, a column out of range, a nonzero
 * pad, an unknown op, RANGE / NOT_RANGE on a byte-array column); also nrules
 * == 0 or > ZP_CLASSIFY_MAX_RULES, a null pointer, a table_bytes too small. */
int zp_classify_compile(const zp_select* rules, uint32_t nrules,
                        void* table /* host */, uint64_t table_bytes);

/* Classifies a parsed batch: one launch on `stream`, nothing allocated,
 * nothing waits, so the call captures into a graph. `table` is the device
 * copy of what zp_classify_compile wrote for the same nrules; `accept` is
 * host memory; everything else device memory.
 * Which frames are read. arena == NULL and offs == NULL is the caller's claim
 * that the table is record-only (zp_classify_compile returned 0): records and
 * lens are streamed and no frame is read; lens may then be NULL too when
 * hits is NULL and no rule bounds the length. A table that reads frames
 * (compile returned 1) needs arena, offs and lens. A record-only table may
 * also be given with all three; it is then evaluated without reading a frame.
 * status (required, one device word). The kernel first checks the table
 * header's signature, version and nrules, and the claims above (record-only
 * against a table with terms; no lens against a table with length bounds).
 * On a mismatch it writes status = 1 and nothing else anywhere, and reads
 * nothing of the table behind the header: a table compiled for another count,
 * one never written. Otherwise status = 0. n == 0 writes status only.
 * Every rule_of[i], i < n, is written and nothing at or past n; mask words
 * [0, ceil(n / 64)); hits entries are only added to (one 64-bit atomic add
 * per workgroup and non-zero entry).
 * Refused with a negative value before any HIP call (zp_last_error names the
 * cause): a null records, table or status; nrules out of range; table_bytes
 * below zp_classify_table_bytes(nrules); n >= 2^32; table, hits, mask or
 * status not 8-byte aligned, rule_of not 4-byte aligned; hits without lens;
 * one of arena / offs given without the other or without lens. */
int zp_classify_device(const uint8_t* arena, const uint64_t* offs, const uint32_t* lens,
                       const zp_record* records, uint64_t n,
                       const void* table /* device copy of the compiled table */,
                       uint64_t table_bytes, uint32_t nrules,
                       const uint64_t* accept /* host, optional */,
                       uint32_t* rule_of /* optional, n */, zp_rule_hits* hits /* optional, nrules+1 */,
                       uint64_t* mask /* optional, ceil(n/64) */,
                       uint64_t* status /* required, 1 device word */, void* stream);

/* ------------------------------------------------------------------------- */
/* Route: longest-prefix match of a frame's address against a table of up to  */
/* ZP_ROUTE_MAX_PREFIXES prefixes (a forwarding table, a blocklist).          */
/*                                                                            */
/* Routed frames. Frame i is looked up when its record has err == 0 and an    */
/*   outer IPv4 or IPv6 reader, and, if `only` (the words zp_select_device    */
/*   writes) is given, bit i % 64 of only[i / 64] is set. Every other frame   */
/*   gets ZP_ROUTE_NONE. The address and its version are exactly the entries  */
/*   zp_extract_columns_device would store for `col` (ZP_COL_DEST_ADDR or     */
/*   ZP_COL_SRC_ADDR) and for ZP_COL_IP_VERSION: under IP-in-IP the outer     */
/*   header's.                                                                */
/* Result. value_of[i] is the `value` of the longest prefix of the frame's    */
/*   version whose first `len` bits equal the address's, ZP_ROUTE_NONE when   */
/*   no prefix matches. The version is part of the match: 10.0.0.1 never      */
/*   matches the IPv6 prefix 0a00:1::/32, and a default route (len 0) of      */
/*   version 4 does not cover IPv6 frames.                                    */
/* Mask. The words zp_select_device writes (bit i % 64 of word i / 64, bits   */
/*   at and past n zero): frame i's bit is set when value_of[i] is not        */
/*   ZP_ROUTE_NONE. zp_select_device's consumers and both flow entry points   */
/*   take it. `mask` and `only` must not overlap.                             */
/* ------------------------------------------------------------------------- */
#define ZP_ROUTE_NONE         0xFFFFFFFFu
#define ZP_ROUTE_VALUE_MAX    0x7FFFFFFEu
#define ZP_ROUTE_MAX_PREFIXES (1u << 20)
typedef struct zp_route_prefix {   /* 24 bytes */
    uint8_t  addr[16];  /* as the address columns hold it: IPv4 in bytes 0-3, zeros behind */
    uint8_t  len;       /* 0..32 for version 4, 0..128 for version 6; 0 = default route */
    uint8_t  version;   /* 4 or 6 */
    uint8_t  pad[2];    /* must be 0 */
    uint32_t value;     /* caller's next hop / class id, <= ZP_ROUTE_VALUE_MAX */
} zp_route_prefix;

/* Exact bytes of the compiled form of p[0, n) (host; n == 0: the empty table,
 * p may be NULL); 0 when zp_route_compile would refuse the prefixes
 * (zp_last_error names the cause). The form is a leaf-pushed multibit trie:
 * one root of 65,536 dword entries per version, then 1-KiB nodes of 256
 * entries, so IPv4 is answered after at most 3 dependent loads and IPv6
 * after at most 15. The size is at most
 *   64 + 512 KiB + 1 KiB * sum over the prefixes of max(0, ceil((len - 16) / 8))
 * bytes (prefixes that share leading bytes share nodes); the caller decides
 * whether that fits. */
uint64_t zp_route_table_bytes(const zp_route_prefix* p, uint32_t n);

/* Compiles p[0, n) into `table` (host memory, 4-byte aligned, table_bytes >=
 * zp_route_table_bytes(p, n)): a private, versioned form the caller copies to
 * the device as it is; the library allocates no device memory and this call
 * touches no device. The same set of prefixes in any order gives the same
 * zp_route_table_bytes(p, n) bytes (padding is zero; nothing behind them is
 * written), so tables can be compared and cached. n == 0 is the empty table:
 * everything routes to ZP_ROUTE_NONE. Returns 0.
 * Refused with a negative value, `table` untouched and zp_last_error naming
 * the prefix index and the cause: n above ZP_ROUTE_MAX_PREFIXES; a version
 * other than 4 or 6; a len past the version's width; a nonzero pad; a value
 * above ZP_ROUTE_VALUE_MAX; address bits set past len (for version 4 also
 * past byte 3); two prefixes with the same (version, len, addr), both
 * indices named; a null pointer; a misaligned table; a table_bytes too small. */
int zp_route_compile(const zp_route_prefix* p, uint32_t n, void* table /* host */,
                     uint64_t table_bytes);

/* One address through a compiled table on the host: the walk the kernel
 * runs. table_bytes is the table's own size (zp_route_table_bytes); addr as
 * in zp_route_prefix (version 4 reads bytes 0-3). ZP_ROUTE_NONE for a table
 * whose header does not say that, and for a version other than 4 or 6.
 * Whatever the bytes behind a valid header hold, the walk makes at most 3
 * (version 4) or 15 (version 6) loads, all inside [table, table + table_bytes). */
uint32_t zp_route_lookup_host(const void* table, uint64_t table_bytes, const uint8_t addr[16],
                              int version);

/* Routes a parsed batch: one launch on `stream`, nothing allocated, nothing
 * waits, so the call captures into a graph. `table` is the device copy of
 * what zp_route_compile wrote and table_bytes its size
 * (zp_route_table_bytes); everything else is device memory too.
 * status (required, one device word). The kernel first checks the table
 * header: signature, version, and the byte size against table_bytes. On a
 * mismatch it writes status = 1 and nothing else anywhere, and reads nothing
 * of the table behind the header. Otherwise status = 0. n == 0 writes status
 * only. Every value_of[i], i < n, is written and nothing at or past n; mask
 * words [0, ceil(n / 64)).
 * Refused with a negative value before any HIP call (zp_last_error names the
 * cause): a null records, table or status; col not ZP_COL_DEST_ADDR or
 * ZP_COL_SRC_ADDR; arena, offs or lens missing; n >= 2^32; a table_bytes
 * below an empty table's; table, only, mask or status not 8-byte aligned,
 * value_of not 4-byte aligned; mask overlapping only. */
int zp_route_device(const uint8_t* arena, const uint64_t* offs, const uint32_t* lens,
                    const zp_record* records, uint64_t n,
                    const void* table /* device copy of the compiled table */, uint64_t table_bytes,
                    int col /* ZP_COL_DEST_ADDR or ZP_COL_SRC_ADDR */,
                    const uint64_t* only /* optional, select's mask words */,
                    uint32_t* value_of /* optional, n */, uint64_t* mask /* optional, ceil(n/64) */,
                    uint64_t* status /* required, 1 device word */, void* stream);

/* ------------------------------------------------------------------------- */
/* Flow table: group parsed frames by key on the device, with per-flow        */
/* counters. zp_stats_device counts per batch; this counts per key.           */
/*                                                                            */
/* Keyed frames. Frame i is keyed when its record has err == 0 and an outer   */
/*   IPv4 or IPv6 reader, and, if `mask` (the words zp_select_device writes)  */
/*   is given, bit i % 64 of mask[i / 64] is set. Every other frame is not    */
/*   keyed: its flow_of[i] is ZP_FLOW_NONE and it contributes to nothing.     */
/* Key. The 40-byte zp_flow_key, built only from the entries                  */
/*   zp_extract_columns_device would store for that frame: the outer IP       */
/*   addresses (IPv4 in bytes 0-3, zeros behind) and ip_version always;       */
/*   key_flags picks the ports (ZP_FLOW_PORTS; 0 without TCP / UDP), l4_proto */
/*   (ZP_FLOW_PROTO) and the VLAN id, ZP_COL_VLAN_TCI & 0x0FFF                */
/*   (ZP_FLOW_VLAN); a field that is not picked is 0. The 5-tuple is          */
/*   ZP_FLOW_PORTS | ZP_FLOW_PROTO. ip_version is part of the key, so         */
/*   10.0.0.1 and the IPv6 address 0a00:0001:: are different flows. Under     */
/*   ip_in_ip the key holds the OUTER addresses and the INNERMOST L4 ports    */
/*   and l4_proto, exactly as the columns do.                                 */
/* ZP_FLOW_BIDIR. Both directions are one flow: if (src_addr bytes, then      */
/*   src_port as a number) is greater than (dest_addr bytes, dest_port),      */
/*   compared lexicographically, the two endpoints are swapped in the key     */
/*   (the ports are compared as the key holds them: 0 without ZP_FLOW_PORTS). */
/*   Equal endpoints stay as they are.                                        */
/* Flow numbering. With F distinct keys among the keyed frames, flows are     */
/*   numbered 0..F-1 in ascending order of their first frame (the smallest i  */
/*   that has the key). The table is filled in whatever order the hardware    */
/*   runs the frames; this numbering makes every output deterministic.        */
/* ------------------------------------------------------------------------- */
#define ZP_FLOW_PORTS 1u
#define ZP_FLOW_PROTO 2u
#define ZP_FLOW_VLAN  4u
#define ZP_FLOW_BIDIR 8u
#define ZP_FLOW_NONE  0xFFFFFFFFu
typedef struct zp_flow_key {         /* 40 bytes */
    uint8_t  src_addr[16], dest_addr[16];   /* ZP_COL_SRC_ADDR / ZP_COL_DEST_ADDR            */
    uint16_t src_port, dest_port;    /* ZP_COL_SRC_PORT / ZP_COL_DEST_PORT   ZP_FLOW_PORTS   */
    uint8_t  l4_proto;               /* ZP_COL_L4_PROTO                      ZP_FLOW_PROTO   */
    uint8_t  ip_version;             /* ZP_COL_IP_VERSION, always part of the key            */
    uint16_t vlan;                   /* ZP_COL_VLAN_TCI & 0x0FFF             ZP_FLOW_VLAN    */
} zp_flow_key;
typedef struct zp_flow_entry {       /* 64 bytes */
    zp_flow_key key;
    uint32_t first, last;            /* the flow's first and last frame index                */
    uint32_t packets;
    uint8_t  tcp_flags;              /* OR of ZP_COL_TCP_FLAGS over the flow's frames        */
    uint8_t  pad[3];                 /* 0                                                    */
    uint64_t bytes;                  /* sum of lens                                          */
} zp_flow_entry;
typedef struct zp_flow_opts {        /* host memory */
    uint32_t key_flags;              /* ZP_FLOW_*                                            */
    uint32_t pad;                    /* must be 0                                            */
    uint64_t max_flows;              /* capacity of `flows`, > 0                             */
    uint64_t hash_mask;              /* UINT64_MAX. The key's hash is ANDed with it before   */
} zp_flow_opts;                      /* any use; tests pass small values to force collisions */

/* Bytes of device scratch zp_flow_aggregate_device needs: 48 B per frame (the
 * key, its slot and TCP flags), one bit and 4 B per 256 frames for the ranking,
 * and 8 B per slot of a table of the first power of two >= 2 * min(max_flows, n)
 * slots (at least 64), plus less than 2 KiB. That is below 64 B per frame +
 * 64 B per max_flows + 4,096 B. */
uint64_t zp_flow_scratch_bytes(uint64_t n, uint64_t max_flows);

/* Groups the keyed frames of a parsed batch by key. `opts` is host memory,
 * everything else device memory:
 *   mask     optional, ceil(n / 64) words as zp_select_device writes them;
 *   flow_of  optional, n entries: frame i's flow number, or ZP_FLOW_NONE;
 *   flows    required, max_flows entries: flows[f] for f < F; `first` and `last`
 *            are frame indices, entries at and past F are not written;
 *   count    required, 4 words: {F, keyed frames, keyed bytes, overflow}.
 *            overflow is 1 exactly when F > max_flows; then only count[3] is
 *            defined, and still nothing is written outside the stated
 *            capacities.
 * Flows are told apart by comparing the whole key, never by its hash, so the
 * results do not depend on hash_mask. The call clears what it needs of
 * `scratch` itself, on the stream: scratch of any prior content gives the same
 * result. Refused with a negative value before anything is launched
 * (zp_last_error names the cause): a null opts, records, lens, arena, offs,
 * flows, count or scratch, unknown key_flags bits, a nonzero pad, max_flows ==
 * 0, n >= 2^32, min(max_flows, n) > 2^30, a misaligned pointer (flows, count,
 * mask: 8 B; flow_of: 4 B), scratch_bytes below zp_flow_scratch_bytes(n,
 * max_flows). n == 0 writes count = {0, 0, 0, 0} and returns 0.
 * Six kernel launches on `stream` (key, insert, mark, scan, heads, label;
 * a second scan launch past ZP_SELECT_SCAN_FRAMES frames); nothing is allocated and nothing waits, so the call captures into a
 * graph. */
int zp_flow_aggregate_device(const uint8_t* arena, const uint64_t* offs, const uint32_t* lens,
                             const zp_record* records, uint64_t n,
                             const zp_flow_opts* opts /* host */,
                             const uint64_t* mask /* optional */,
                             uint32_t* flow_of /* optional: n entries */,
                             zp_flow_entry* flows /* required: max_flows entries */,
                             uint64_t* count /* required: 4 device words */,
                             void* scratch, uint64_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------------- */
/* Persistent flow table: the same grouping, kept across batches.             */
/*                                                                            */
/* A flow table is two pieces of caller-owned device memory: a `table` block  */
/* of zp_flow_table_bytes(max_flows) bytes (a 64-byte header and the hash     */
/* slots) and `flows`, max_flows zp_flow_state entries. The options are fixed */
/* when the table is initialised: every later call must pass the same         */
/* key_flags, max_flows and hash_mask. The library allocates nothing, waits   */
/* for nothing and reads nothing back: every call is enqueue-only on the      */
/* caller's stream and captures into a graph. One table is used from one      */
/* stream at a time.                                                          */
/*                                                                            */
/* Epoch. The header holds `epoch`, the number of updates completed (0 after  */
/*   init). Update number E, counted from 0, stamps what it touches with E    */
/*   (its low 32 bits) and its last launch writes epoch = E + 1. The counter  */
/*   lives on the device, so a replayed graph advances it.                    */
/* Update. Which frames are keyed, and their keys, are exactly                */
/*   zp_flow_aggregate_device's (same rule, mask and key_flags). With F0 the  */
/*   table's flow count before the call:                                      */
/*   1. a keyed frame whose key is in the table belongs to that flow;         */
/*   2. the remaining keyed frames are grouped among themselves; their R      */
/*      distinct keys are ranked 0..R-1 in ascending order of their first     */
/*      frame in this batch. New key r is ADMITTED as flow F0 + r when        */
/*      F0 + r < max_flows and REFUSED otherwise: a refused key's frames get  */
/*      ZP_FLOW_NONE, contribute to no entry, and nothing of the key enters   */
/*      the table, so a full table stays valid;                               */
/*   3. an admitted flow's entry is {key, first_epoch = last_epoch = E, 0s};  */
/*   4. every keyed frame that is not refused adds 1 to its flow's packets    */
/*      and lens[i] to its bytes, ORs its TCP flags in, and sets last_epoch   */
/*      = E.                                                                  */
/*   Every output byte is the same whatever order the hardware runs in.       */
/* Retire. With E the header's epoch, flow f is retired when                  */
/*   max_idle != ZP_FLOW_IDLE_NEVER and E - 1 - last_epoch >= max_idle (the   */
/*   left side is the number of updates since the one that last saw the flow; */
/*   0 retires everything), or when ZP_FLOW_STATE_TCP_FLAGS & tcp_any != 0.   */
/*   Survivors are compacted stably to flows[0, F') byte for byte, so flows   */
/*   stay numbered in order of first appearance.                              */
/* ------------------------------------------------------------------------- */
#define ZP_FLOW_IDLE_NEVER 0xFFFFFFFFu
typedef struct zp_flow_state {       /* 64 bytes */
    zp_flow_key key;                 /* as zp_flow_aggregate_device builds it                */
    uint32_t first_epoch, last_epoch;/* the updates that admitted and last saw the flow      */
    uint64_t packets_flags;          /* bits 0-55 packets, bits 56-63 OR of the TCP flags    */
    uint64_t bytes;                  /* sum of lens                                          */
} zp_flow_state;
#define ZP_FLOW_STATE_PACKETS(e)   ((e).packets_flags & 0x00FFFFFFFFFFFFFFull)
#define ZP_FLOW_STATE_TCP_FLAGS(e) ((uint8_t)((e).packets_flags >> 56))

/* Bytes of the `table` block: a 64-byte header and one 4-byte slot for each of
 * the first power of two >= 2 * max_flows slots (at least 64): at most 16 B per
 * max_flows + 512 B. max_flows above 2^30 is refused by the calls. */
uint64_t zp_flow_table_bytes(uint64_t max_flows);
/* Device scratch of one update of n frames: zp_flow_aggregate_device's for n
 * frames and n flows, at most 96 B per frame + 4,096 B. */
uint64_t zp_flow_update_scratch_bytes(uint64_t n);
/* Device scratch of a retire: a staging copy of the survivors and the ranking,
 * at most 72 B per max_flows + 4,096 B. */
uint64_t zp_flow_retire_scratch_bytes(uint64_t max_flows);

/* Writes the table's header (a signature of `opts`, F = 0, epoch = 0) and
 * empties the slots; `flows` is not touched. One launch. Refused (negative,
 * zp_last_error names the cause): null opts or table, unknown key_flags bits,
 * a nonzero pad, max_flows == 0 or above 2^30, a misaligned table (8 B),
 * table_bytes below zp_flow_table_bytes(max_flows). */
int zp_flow_table_init_device(void* table, uint64_t table_bytes, const zp_flow_opts* opts /* host */,
                              void* stream);

/* One update of the table by a parsed batch (the rule above).
 *   flow_of  optional, n entries: the table-wide flow number, or ZP_FLOW_NONE
 *            (not keyed, or refused);
 *   count    required, 8 words: {F after the call, flows admitted, keyed frames,
 *            keyed bytes, refused flows, refused frames, E, status}. Keyed frames
 *            and bytes count every keyed frame, the refused ones included.
 *            status is 1, and nothing else anywhere is written or changed, when
 *            the header's signature does not match `opts`: a table never
 *            initialised, or initialised with other options. Every kernel of
 *            the call checks the signature first.
 * n == 0 still completes an epoch and writes count. Scratch of any prior
 * content gives the same result. Refused before anything is launched: what
 * zp_flow_aggregate_device refuses, and a null or too small table, n >= 2^31,
 * max_flows > 2^30, scratch_bytes below zp_flow_update_scratch_bytes(n), a
 * misaligned pointer (table, count, mask: 8 B; flows: 16 B; flow_of: 4 B).
 * Seven launches (key, find + insert, mark, scan, admit, label, finish; a
 * second scan launch past ZP_SELECT_SCAN_FRAMES frames); one with n == 0. */
int zp_flow_update_device(const uint8_t* arena, const uint64_t* offs, const uint32_t* lens,
                          const zp_record* records, uint64_t n,
                          const zp_flow_opts* opts /* host */, const uint64_t* mask /* optional */,
                          void* table, uint64_t table_bytes,
                          zp_flow_state* flows /* max_flows entries */,
                          uint32_t* flow_of /* optional: n entries */,
                          uint64_t* count /* required: 8 device words */,
                          void* scratch, uint64_t scratch_bytes, void* stream);

/* Retires flows by the two predicates above (tcp_any: a mask of TCP flag bits,
 * at most 0xFF; 0 for none).
 *   retired  optional, max_flows entries: the retired entries in ascending old
 *            number (the export record);
 *   remap    optional, max_flows words: remap[f] for f below the old F is the
 *            flow's new number, or ZP_FLOW_NONE; words past the old F are not
 *            written;
 *   count    required, 2 words: {F', flows retired}. On a signature mismatch
 *            count[1] = UINT64_MAX and nothing else is written.
 * The slots are rebuilt from the survivors, the header gets F = F', epoch is
 * untouched, entries of `flows` at and past F' are left as they are. Refused
 * before anything is launched: null opts, table, flows, count or scratch, bad
 * opts as for init, tcp_any above 0xFF, a too small table or scratch (below
 * zp_flow_retire_scratch_bytes(max_flows)), a misaligned pointer (table, count:
 * 8 B; flows, retired: 16 B; remap: 4 B). Six launches (mark, scan, move,
 * copy back + clear, re-insert, finish; a second scan launch past
 * ZP_SELECT_SCAN_FRAMES flows). */
int zp_flow_retire_device(const zp_flow_opts* opts /* host */, void* table, uint64_t table_bytes,
                          zp_flow_state* flows, uint32_t max_idle, uint32_t tcp_any,
                          zp_flow_state* retired /* optional */, uint32_t* remap /* optional */,
                          uint64_t* count /* required: 2 device words */,
                          void* scratch, uint64_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------------- */
/* Batched PacketBuilder. The reference builds one    */
/* frame with a typestate chain over a caller-sized buffer                    */
/* (builder.rs:55-909): PacketBuilder::new(&mut buf).ethernet(..).ipv4(..)    */
/* .tcp(..).build(). Here every frame of a batch carries its chain as a run   */
/* of zp_build_op (one op per builder method, in call order) and the kernel   */
/* executes all chains in place over the frames' buffers, with the writers'   */
/* exact byte semantics: read-modify-write of shared bytes, checksums over    */
/* the whole remaining buffer, and the first Err stopping the chain with the  */
/* partial writes left in place, as the reference leaves them.                */
/* A chain that the typestate graph (builder.rs:817-909) would not compile    */
/* is refused before anything is written (ZP_BERR_TRANSITION); a chain whose  */
/* reference run would panic reports ZP_BERR_PANIC.                           */
/* ------------------------------------------------------------------------- */
typedef enum zp_build_kind {
    ZP_B_ETHERNET = 1,       /* builder.rs:113  src=src_mac dst=dest_mac h0=ethertype      */
    ZP_B_ETHERNET_VLAN = 2,  /* builder.rs:141  + h1=tci                                    */
    ZP_B_ETHERNET_QINQ = 3,  /* builder.rs:171  + h1=tci1 h2=tci2                           */
    ZP_B_ARP = 4,            /* builder.rs:203  h0=htype h1=ptype b0=hlen b1=plen h2=oper   */
                             /*   src[0:6]=sha src[6:10]=spa dst[0:6]=tha dst[6:10]=tpa      */
    ZP_B_IPV4 = 5,           /* builder.rs:248/343 b0=version b1=ihl b2=dscp b3=ecn          */
                             /*   h0=total_length h1=identification b4=flags h2=fragment_offset */
                             /*   b5=ttl b6=protocol src[0:4]=src_ip dst[0:4]=dest_ip          */
    ZP_B_IPV6 = 6,           /* builder.rs:300/395 b0=version b1=traffic_class w0=flow_label */
                             /*   h0=payload_length b2=next_header b3=hop_limit src dst      */
    ZP_B_HOP_BY_HOP = 7,     /* builder.rs:611  b0=next_header b1=extension_len data=options */
    ZP_B_DEST_OPTS1 = 8,     /* builder.rs:643  as hop_by_hop                               */
    ZP_B_ROUTING = 9,        /* builder.rs:675  b0=next_header b1=header_ext_len            */
                             /*   b2=routing_type b3=segments_left data=data                 */
    ZP_B_FRAGMENT = 10,      /* builder.rs:711  b0=next_header h0=fragment_offset b1=m_flag */
                             /*   w0=identification                                          */
    ZP_B_AUTH = 11,          /* builder.rs:747  b0=next_header b1=payload_len w0=spi        */
                             /*   w1=seq_num data=auth_data                                  */
    ZP_B_DEST_OPTS2 = 12,    /* builder.rs:785  as hop_by_hop                               */
    ZP_B_TCP = 13,           /* builder.rs:438  src/dst = pseudo-header addresses (4 B      */
                             /*   under IPv4 states, 16 B otherwise) h0=src_port h1=dest_port */
                             /*   w0=sequence_number w1=acknowledgment_number b0=data_offset  */
                             /*   b1=reserved b2=flags h2=window_size h3=urgent_pointer      */
                             /*   data=payload (optional)                                    */
    ZP_B_UDP = 14,           /* builder.rs:492  src/dst h0=src_port h1=dest_port h2=length  */
                             /*   data=payload (optional)                                    */
    ZP_B_ICMPV4 = 15,        /* builder.rs:534  b0=icmp_type b1=icmp_code data=payload (opt) */
    ZP_B_ICMPV6 = 16,        /* builder.rs:571  src/dst b0=icmp_type b1=icmp_code data (opt) */
    ZP_B_KIND_COUNT = 17
} zp_build_kind;

#define ZP_BUILD_NO_DATA 0xFFFFFFFFu   /* data_len: payload None (others: empty)   */

typedef struct zp_build_op {           /* 64 bytes */
    uint8_t  kind;                     /* zp_build_kind                            */
    uint8_t  b[7];
    uint16_t h[4];
    uint32_t w[2];
    uint32_t data_off;                 /* variable bytes at data + data_off        */
    uint32_t data_len;                 /* ... their length, or ZP_BUILD_NO_DATA    */
    uint8_t  src[16];
    uint8_t  dst[16];
} zp_build_op;

typedef enum zp_build_err {
    ZP_BUILD_OK = 0,
    ZP_BERR_ETH_SLICE = 1,            /* ethernet.rs:30                            */
    ZP_BERR_ETH_VLAN = 2,             /* ethernet.rs:85                            */
    ZP_BERR_ETH_QINQ = 3,             /* ethernet.rs:112                           */
    ZP_BERR_ARP_DATA = 4,             /* builder.rs:216                            */
    ZP_BERR_ARP_SLICE = 5,            /* arp.rs:17                                 */
    ZP_BERR_IPV4_DATA = 6,            /* builder.rs:264,359                        */
    ZP_BERR_IPV4_SLICE = 7,           /* ipv4.rs:18                                */
    ZP_BERR_IPV6_DATA = 8,            /* builder.rs:312,407                        */
    ZP_BERR_IPV6_SLICE = 9,           /* ipv6.rs:18                                */
    ZP_BERR_TCP_DATA = 10,            /* builder.rs:454                            */
    ZP_BERR_TCP_SLICE = 11,           /* tcp.rs:17                                 */
    ZP_BERR_TCP_PAYLOAD = 12,         /* tcp.rs:110 == udp.rs:84                   */
    ZP_BERR_UDP_DATA = 13,            /* builder.rs:502                            */
    ZP_BERR_UDP_SLICE = 14,           /* udp.rs:17                                 */
    ZP_BERR_ICMPV4_DATA = 15,         /* builder.rs:541                            */
    ZP_BERR_ICMP_SLICE = 16,          /* icmpv4.rs:20 == icmpv6.rs:17              */
    ZP_BERR_ICMPV4_PAYLOAD = 17,      /* icmpv4.rs:61                              */
    ZP_BERR_ICMPV6_DATA = 18,         /* builder.rs:580                            */
    ZP_BERR_ICMPV6_PAYLOAD = 19,      /* icmpv6.rs:58                              */
    ZP_BERR_HBH_DATA = 20,            /* builder.rs:618                            */
    ZP_BERR_DEST_DATA = 21,           /* builder.rs:650,792                        */
    ZP_BERR_OPTIONS_SLICE = 22,       /* options.rs:18                             */
    ZP_BERR_OPTIONS_MIN = 23,         /* options.rs:54                             */
    ZP_BERR_OPTIONS_MATCH = 24,       /* options.rs:60                             */
    ZP_BERR_OPTIONS_EXCEED = 25,      /* options.rs:67                             */
    ZP_BERR_ROUTING_DATA = 26,        /* builder.rs:684,719 (fragment_header too)  */
    ZP_BERR_ROUTING_SLICE = 27,       /* routing.rs:16                             */
    ZP_BERR_ROUTING_MIN = 28,         /* routing.rs:77                             */
    ZP_BERR_ROUTING_MATCH = 29,       /* routing.rs:83                             */
    ZP_BERR_ROUTING_EXCEED = 30,      /* routing.rs:90                             */
    ZP_BERR_AUTH_DATA = 31,           /* builder.rs:756                            */
    ZP_BERR_AUTH_SLICE = 32,          /* authentication.rs:16                      */
    ZP_BERR_AUTH_EXCEED = 33,         /* authentication.rs:88                      */
    ZP_BERR_PANIC = 34,               /* the reference would panic: fragment.rs:16 */
                                      /* panic!, or a slice index out of range      */
                                      /* (ipv4.rs:123, tcp.rs:114)                  */
    ZP_BERR_TRANSITION = 35,          /* chain not allowed by builder.rs:817-909    */
    ZP_BERR_COUNT = 36
} zp_build_err;

typedef struct zp_build_result {
    uint32_t header_len;               /* PacketBuilder::header_len() (builder.rs:65) */
    uint8_t  err;                      /* zp_build_err                             */
    uint8_t  ops_done;                 /* ops that returned Ok                     */
    uint16_t reserved;
} zp_build_result;

/* Exact reference string of a zp_build_err ("" for OK, NULL out of range). */
const char* zp_build_err_str(int code);

/* Runs n builder chains in place on the device. Frame i is the buffer
 * arena[offs[i] .. offs[i] + lens[i]) (the reference's `&mut [u8]`), its
 * chain is ops[op_start[i] .. op_start[i + 1]) (op_start has n + 1 entries),
 * variable bytes come from `data`. results may be NULL. All pointers are
 * device memory; enqueues on `stream`. Returns 0 or negative on failure.
 * Precondition (not checked on the device, as for zp_parse_batch_device):
 * every frame lies inside the arena, the frames do not overlap (the kernel
 * writes them), every op's data range lies inside `data`. The Python API
 * (BuildBatch.run) checks the descriptors first. */
int zp_build_batch_device(uint8_t* arena, const uint64_t* offs, const uint32_t* lens,
                          uint64_t n, const zp_build_op* ops, const uint32_t* op_start,
                          const uint8_t* data, zp_build_result* results, void* stream);

/* The same over host buffers (a transmit ring), through `ctx`: the frames'
 * bytes go H2D, the chains run, the frame bytes come back. data_bytes is the
 * size of the data blob. Synchronous. Returns 0 or negative on failure. */
int zp_build_batch_host(zp_ctx* ctx, uint8_t* arena, uint64_t arena_bytes,
                        const uint64_t* offs, const uint32_t* lens, uint64_t n,
                        const zp_build_op* ops, const uint32_t* op_start,
                        const uint8_t* data, uint64_t data_bytes, zp_build_result* results);

/* ------------------------------------------------------------------------- */
/* Synthetic batch generator (BASELINE.json configs 1-5, mixed config 6),    */
/* built from the builder's checksum-fill semantics                          */
/* (builder.rs:473-474,515-516,553,592-593).                                 */
/* Deterministic per packet: packet i depends only on (config, seed, i).      */
/* ------------------------------------------------------------------------- */
#define ZP_CFG_C1_ETH_IPV4_UDP_64 1  /* == C2 layout, CPU plumbing            */
#define ZP_CFG_C2_ETH_IPV4_UDP_64 2
#define ZP_CFG_C3_IPV4_MIX        3
#define ZP_CFG_C4_IPV6_EXT_VLAN   4
#define ZP_CFG_C5_IMIX_IPINIP     5
#define ZP_CFG_C6_MIXED           6  /* not a BASELINE config: per packet the shape
                                        of C3, C4 or C5 (5/16 each) or a 64-B ARP
                                        frame (1/16), so every tile mixes stacks */
#define ZP_GEN_SEED_DEFAULT 0x5EED2025ull

/* Frame length of packet `first + i`, i in [0, n), into d_lens (device). */
int zp_gen_lengths_device(int config, uint64_t seed, uint64_t first, uint64_t n,
                          uint32_t* lens, void* stream);
/* Writes frame `first + i` at arena + offs[i] (offs/lens device arrays as
 * produced by zp_gen_lengths_device + an exclusive scan). */
int zp_gen_frames_device(int config, uint64_t seed, uint64_t first, uint64_t n,
                         uint8_t* arena, const uint64_t* offs,
                         const uint32_t* lens, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* ZERO_PACKET_H */
