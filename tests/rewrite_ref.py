"""Plain-Python restatement of zp_rewrite_columns_device over one frame
(include/zero_packet.h, semantics 1-5): the writers' setters applied to a
bytearray, then both checksums recomputed IN FULL with the oracle's
internet_checksum / pseudo_header, the way IPv4Writer::set_checksum
(ipv4.rs:119-126) and the L4 writers' set_checksum(pseudo_sum)
(tcp.rs:123-129, udp.rs:65-71, icmpv4.rs:74-80, icmpv6.rs:71-77) do it.
Nothing here is incremental, so it is independent of the kernel's arithmetic.
Offsets and presence come from the oracle's record (test infrastructure).
"""
import oracle as orc
from fuzzfix import _ext_end

F_ETHERNET, F_IPV4, F_IPV6, F_IP_IN_IP, F_IP_IN_IP_V6 = 1, 4, 8, 16, 32
F_TCP, F_UDP, F_ICMPV4, F_ICMPV6 = 64, 128, 256, 512
L4_MASK = F_TCP | F_UDP | F_ICMPV4 | F_ICMPV6

WRITABLE = ("dest_mac", "src_mac", "vlan_tci", "vlan_inner_tci", "src_addr", "dest_addr", "ttl",
            "tos", "ip_id", "src_port", "dest_port", "tcp_seq", "tcp_ack", "tcp_window")
NAT = ("src_addr", "dest_addr", "src_port", "dest_port", "ttl")


def _be(v, n):
    return int(v).to_bytes(n, "big")


def _innermost(f, rec, ext):
    """(src, dst, protocol, is_v4) of the IP header whose payload starts at the
    record's l4_off: the reader that verified the L4 checksum (parser.rs:111-135)."""
    hl, l4 = int(rec["eth_len"]), int(rec["l4_off"])
    flags = int(rec["flags"])
    if not flags & F_IP_IN_IP:
        if flags & F_IPV4:
            return f[hl + 12:hl + 16], f[hl + 16:hl + 20], f[hl + 9], True
        return f[hl + 8:hl + 24], f[hl + 24:hl + 40], int(rec["final_nh"]), False
    pos, v6, first = int(rec["inner_off"]), bool(flags & F_IP_IN_IP_V6), True
    while pos < l4:
        if v6:
            if first:                       # the record's own chain length and final header
                nxt, proto = pos + 40 + int(ext[1]["len"]), int(rec["inner_final_nh"])
            else:
                nxt, proto = _ext_end(f, pos + 40, f[pos + 6])
            src, dst = f[pos + 8:pos + 24], f[pos + 24:pos + 40]
        else:
            nxt, proto = pos + (f[pos] & 15) * 4, f[pos + 9]
            src, dst = f[pos + 12:pos + 16], f[pos + 16:pos + 20]
        if nxt == l4 and proto not in (4, 41):
            return src, dst, proto, not v6
        assert proto in (4, 41) and nxt > pos, "rewrite_ref: lost the IP-in-IP chain"
        pos, v6, first = nxt, proto == 41, False
    raise AssertionError("rewrite_ref: no IP header ends at l4_off")


def rewrite_ref(frame, rec, ext, w):
    """frame: bytes; rec / ext: the oracle's record of it and its two chain
    entries; w: {column name: value} (MACs / addresses as bytes-likes of 6 /
    16, the rest ints), absent = NULL column. Returns (new frame bytes,
    {name: changed} for every column whose entry applied to this frame)."""
    f = bytearray(frame)
    applied = {}
    flags = int(rec["flags"])
    if int(rec["err"]) or not flags & F_ETHERNET:             # semantics 1
        return bytes(f), applied

    def put(name, x, data):
        data = bytes(data)
        applied[name] = bytes(f[x:x + len(data)]) != data
        f[x:x + len(data)] = data

    hl, l4, n = int(rec["eth_len"]), int(rec["l4_off"]), len(f)
    if "dest_mac" in w:
        put("dest_mac", 0, bytes(w["dest_mac"])[:6])                  # ethernet.rs:47
    if "src_mac" in w:
        put("src_mac", 6, bytes(w["src_mac"])[:6])                    # ethernet.rs:58
    tp = (f[12] << 8) | f[13]
    if "vlan_tci" in w and tp in (0x8100, 0x88A8):                    # ethernet.rs:83-129
        put("vlan_tci", 14, _be(w["vlan_tci"], 2))
    if "vlan_inner_tci" in w and tp == 0x88A8:
        put("vlan_inner_tci", 18, _be(w["vlan_inner_tci"], 2))
    v4, v6 = bool(flags & F_IPV4), bool(flags & F_IPV6)
    if v4:
        if "tos" in w:
            put("tos", hl + 1, [int(w["tos"])])                       # ipv4.rs:46-54
        if "ip_id" in w:
            put("ip_id", hl + 4, _be(int(w["ip_id"]) & 0xFFFF, 2))    # ipv4.rs:67
        if "ttl" in w:
            put("ttl", hl + 8, [int(w["ttl"])])                       # ipv4.rs:87
        if "src_addr" in w:
            put("src_addr", hl + 12, bytes(w["src_addr"])[:4])        # ipv4.rs:99-113
        if "dest_addr" in w:
            put("dest_addr", hl + 16, bytes(w["dest_addr"])[:4])
    elif v6:
        if "tos" in w:                                                # ipv6.rs:42
            tc = int(w["tos"])
            put("tos", hl, [(f[hl] & 0xF0) | (tc >> 4), (f[hl + 1] & 0x0F) | ((tc << 4) & 0xF0)])
        if "ip_id" in w:                                              # ipv6.rs:51
            fl = int(w["ip_id"])
            put("ip_id", hl + 1, [(f[hl + 1] & 0xF0) | ((fl >> 16) & 0x0F), (fl >> 8) & 0xFF,
                                  fl & 0xFF])
        if "ttl" in w:
            put("ttl", hl + 7, [int(w["ttl"])])                       # ipv6.rs:84
        if "src_addr" in w:
            put("src_addr", hl + 8, bytes(w["src_addr"])[:16])        # ipv6.rs:92-133
        if "dest_addr" in w:
            put("dest_addr", hl + 24, bytes(w["dest_addr"])[:16])
    l4f = flags & L4_MASK
    if l4f in (F_TCP, F_UDP):
        if "src_port" in w:
            put("src_port", l4, _be(w["src_port"], 2))                # tcp.rs:37, udp.rs:37
        if "dest_port" in w:
            put("dest_port", l4 + 2, _be(w["dest_port"], 2))
    if l4f == F_TCP:
        if "tcp_seq" in w:
            put("tcp_seq", l4 + 4, _be(w["tcp_seq"], 4))              # tcp.rs:51
        if "tcp_ack" in w:
            put("tcp_ack", l4 + 8, _be(w["tcp_ack"], 4))              # tcp.rs:60
        if "tcp_window" in w:
            put("tcp_window", l4 + 14, _be(w["tcp_window"], 2))       # tcp.rs:87

    # semantics 3: IPv4Writer::set_checksum, unless every covered byte kept its value
    if v4:
        ihl = (f[hl] & 15) * 4
        if bytes(f[hl:hl + 10]) + bytes(f[hl + 12:hl + ihl]) != \
                frame[hl:hl + 10] + frame[hl + 12:hl + ihl]:
            f[hl + 10:hl + 12] = b"\0\0"
            f[hl + 10:hl + 12] = _be(orc.internet_checksum(f[hl:hl + ihl]), 2)
    # ... then the L4 writer's set_checksum(pseudo_sum) over f[l4:], semantics 4
    if l4f:
        ck = l4 + (16 if l4f == F_TCP else 6 if l4f == F_UDP else 2)
        src, dst, proto, inner_v4 = _innermost(f, rec, ext)
        osrc, odst, _, _ = _innermost(bytearray(frame), rec, ext)
        covered = lambda b: bytes(b[l4:ck]) + bytes(b[ck + 2:])
        if covered(f) != covered(frame) or (bytes(src), bytes(dst)) != (bytes(osrc), bytes(odst)):
            acc = 0 if (inner_v4 and proto == 1) else \
                orc.pseudo_header(bytes(src), bytes(dst), proto, n - l4)
            f[ck:ck + 2] = b"\0\0"
            f[ck:ck + 2] = _be(orc.internet_checksum(f[l4:], acc), 2)
    return bytes(f), applied


def rewrite_batch_ref(arena, offs, lens, recs, ext, cols):
    """rewrite_ref over a numpy batch: cols {name: numpy column}. Returns (new
    arena, {name: bool array: applied with a changed value},
    {name: bool array: applied})."""
    import numpy as np
    out = arena.copy()
    n = len(offs)
    changed = {k: np.zeros(n, bool) for k in cols}
    applied = {k: np.zeros(n, bool) for k in cols}
    for i in range(n):
        o, l_ = int(offs[i]), int(lens[i])
        w = {k: (v[i].tobytes() if v.ndim > 1 else int(v[i])) for k, v in cols.items()}
        new, ap = rewrite_ref(arena[o:o + l_].tobytes(), recs[i], ext[:, i], w)
        out[o:o + l_] = np.frombuffer(new, np.uint8)
        for k, ch in ap.items():
            applied[k][i] = True
            changed[k][i] = ch
    return out, changed, applied
