"""Frames of a chosen protocol stack (test infrastructure, no tests).

stack() lays out Ethernet II / 802.1Q / QinQ, up to two IP levels (IPv4 with
any IHL, IPv6 with option headers of any size) and an L4 header, with random
field values and payload; tests/fuzzfix.py repair() then fills every checksum
the way the reference builder does. On top of it:

  code_frame()        one frame of each of the 33 record codes (zp_parse.hip
                      rec_code: Ethernet length x (ARP | IP version x L4 kind))
  code_batch()        the record-code batch of tests/test_gpu_paths.py
  window_families()   frames whose L4 and inner IP headers lie on and past
                      the end of the parse window (112 B from the frame's
                      16-B aligned start)
  place_aligned()     each frame at each of the 16 start alignments mod 16
  short_tail_families()  the same stacks without payload: frames that end
                      before the bytes a column reader asks for
  with_filler()       an arena with the bytes between its frames set
"""
import numpy as np

from fuzzfix import repair

CODE_BASE = 0xC0
L4_PROTO = {"none": 253, "tcp": 6, "udp": 17, "icmpv4": 1, "icmpv6": 58}
L4_KINDS = ("none", "tcp", "udp", "icmpv4", "icmpv6")      # the code's l4 digit
L4_MIN = {"none": 0, "tcp": 20, "udp": 8, "icmpv4": 8, "icmpv6": 8}


def _rand(rng, n):
    return bytearray(rng.integers(0, 256, n, dtype=np.uint8).tobytes())


def ethernet(rng, eth_len, ethertype):
    """14 B, 18 B (802.1Q) or 22 B (QinQ: 0x88A8 then 0x8100) with non-zero
    tag control words."""
    f = _rand(rng, eth_len)
    f[0] &= 0xFE
    if eth_len == 18:
        f[12:14] = b"\x81\x00"
        f[15] |= 1
    elif eth_len == 22:
        f[12:14] = b"\x88\xa8"
        f[15] |= 1
        f[16:18] = b"\x81\x00"
        f[19] |= 1
    else:
        assert eth_len == 14
    f[eth_len - 2:eth_len] = ethertype.to_bytes(2, "big")
    return f


def ipv4(rng, ihl, proto, payload_len):
    """IPv4 header of ihl * 4 bytes (random option bytes past 20); the header
    checksum is left to repair()."""
    h = _rand(rng, ihl * 4)
    h[0] = 0x40 | ihl
    h[1] |= 4
    h[2:4] = (ihl * 4 + payload_len).to_bytes(2, "big")
    h[5] |= 1
    h[8] |= 1
    h[9] = proto
    h[10:12] = b"\0\0"
    return h


def ipv6(rng, next_header, payload_len):
    h = _rand(rng, 40)
    h[0] = 0x60 | (h[0] & 15) | 1
    h[3] |= 1
    h[4:6] = (payload_len & 0xFFFF).to_bytes(2, "big")
    h[6] = next_header
    h[7] |= 1
    return h


def options(rng, next_header, size):
    """A Hop-by-Hop / Destination Options header of `size` bytes (a multiple
    of 8): next header, (size / 8) - 1, random option bytes."""
    assert size >= 8 and size % 8 == 0
    h = _rand(rng, size)
    h[0] = next_header
    h[1] = size // 8 - 1
    return h


def l4_segment(rng, kind, size):
    """An L4 header of `kind` with payload, `size` bytes in all; checksum
    left to repair(). ICMP codes are 1-15 (non-zero, and valid for ICMPv4)."""
    assert size >= L4_MIN[kind]
    s = _rand(rng, size)
    if kind == "tcp":
        s[12] = 0x50 | (s[12] & 15)
        s[13] |= 0x10
    elif kind == "udp":
        s[4:6] = size.to_bytes(2, "big")
    elif kind in ("icmpv4", "icmpv6"):
        s[0] = 8 if kind == "icmpv4" else 128
        s[1] = 1 + s[1] % 15
    return s


def stack(rng, eth_len, levels, l4, size=None, min_payload=0):
    """One frame. levels: the IP headers from the outside in, each ("v4", ihl)
    or ("v6", [(kind, size), ...]) with kind 0 (Hop-by-Hop) or 60
    (Destination Options). l4: a key of L4_PROTO. size: the frame length (a
    random one that fits by default). Returns the frame with valid checksums."""
    hdr = eth_len + sum(lv[1] * 4 if lv[0] == "v4" else 40 + sum(s for _, s in lv[1])
                        for lv in levels)
    least = max(64, hdr + max(L4_MIN[l4], min_payload))
    if size is None:
        size = int(rng.integers(least, max(least, 200) + 1))
    assert size >= least, (size, least)
    f = ethernet(rng, eth_len, 0x0800 if levels[0][0] == "v4" else 0x86DD)
    left = size - eth_len
    for k, lv in enumerate(levels):
        nxt = L4_PROTO[l4] if k + 1 == len(levels) else (4 if levels[k + 1][0] == "v4" else 41)
        if lv[0] == "v4":
            left -= lv[1] * 4
            f += ipv4(rng, lv[1], nxt, left)
        else:
            chain = lv[1]
            left -= 40
            f += ipv6(rng, chain[0][0] if chain else nxt, left)
            for j, (_, s) in enumerate(chain):
                f += options(rng, chain[j + 1][0] if j + 1 < len(chain) else nxt, s)
                left -= s
    f += l4_segment(rng, l4, left)
    assert len(f) == size
    return repair(bytes(f))


def arp_frame(rng, eth_len, size=None):
    """Ethernet + a 28-B ARP body (oper 1 or 2), padded to at least 64 B."""
    size = int(rng.integers(64, 201)) if size is None else size
    f = ethernet(rng, eth_len, 0x0806) + _rand(rng, size - eth_len)
    f[eth_len + 6:eth_len + 8] = int(rng.integers(1, 3)).to_bytes(2, "big")
    return bytes(f)


def valid_codes():
    """The 33 record codes: ARP carries no L4 reader."""
    return [CODE_BASE + x for x in range(45) if x // 5 % 3 or x % 5 == 0]


def code_frame(rng, code):
    """A 64-200 B frame whose record has exactly this code: Ethernet length
    14 + 4 * (x / 15), ARP / IPv4 (20-B header) / IPv6 (no extensions) by
    x / 5 % 3, the L4 reader by x % 5 (none: protocol 253)."""
    x = code - CODE_BASE
    eth_len, l3, l4 = 14 + 4 * (x // 15), x // 5 % 3, L4_KINDS[x % 5]
    if l3 == 0:
        assert l4 == "none"
        return arp_frame(rng, eth_len)
    return stack(rng, eth_len, [("v4", 5) if l3 == 1 else ("v6", [])], l4)


ANOMALIES = ("ihl6", "hbh8", "ipip", "l4sum", "v4sum", "cut40", "empty", "giant", "far")
ANOMALY_LANES = (0, 3, 63)
CODE_PREFIXES = (64 * 15, 64 * 16, 64 * 16 + 1, 64 * 17, 64 * 63, 64 * 64, 64 * 65 + 5)


def anomaly_frame(rng, kind, giant, far):
    """A frame that cannot have a record code, of one kind of ANOMALIES.
    giant / far: the long frames (built once by the caller)."""
    eth_len = int(rng.choice([14, 18, 22]))
    l4 = str(rng.choice(["tcp", "udp"]))
    if kind == "ihl6":
        return stack(rng, eth_len, [("v4", 6)], l4)
    if kind == "hbh8":
        return stack(rng, eth_len, [("v6", [(0, 8)])], l4)
    if kind == "ipip":
        return stack(rng, eth_len, [("v4", 5), ("v6", [])], l4)
    if kind == "l4sum":
        f = bytearray(stack(rng, eth_len, [("v6", [])], l4))
        f[-1] ^= 0x20
        return bytes(f)
    if kind == "v4sum":
        f = bytearray(stack(rng, eth_len, [("v4", 5)], l4))
        f[eth_len + 10] ^= 0x04
        return bytes(f)
    if kind == "cut40":
        return stack(rng, eth_len, [("v4", 5)], l4)[:40]
    if kind == "empty":
        return b""
    return {"giant": giant, "far": far}[kind]


def code_batch(rng, giant, far, giant_ok):
    """The record-code batch: 33 tiles of one code each, 33 tiles of 64
    random codes, one tile of coded frames per anomaly kind and lane with the
    anomaly at that lane, one all-coded tile with the accepted long frame
    `giant_ok` at lane 3, and a ragged tail of 37 coded frames. giant: a
    70,001-B frame with a failing checksum; far: a far-L4 frame. Returns
    (frames, want) with want[i] the intended code of frame i (0: none)."""
    codes = valid_codes()
    frames, want = [], []

    def coded(c):
        frames.append(code_frame(rng, c))
        want.append(c)
    for c in codes:
        for _ in range(64):
            coded(c)
    for _ in range(33 * 64):
        coded(int(rng.choice(codes)))
    for kind in ANOMALIES:
        for lane in ANOMALY_LANES:
            for k in range(64):
                if k == lane:
                    frames.append(anomaly_frame(rng, kind, giant, far))
                    want.append(0)
                else:
                    coded(int(rng.choice(codes)))
    for k in range(64):
        if k == 3:
            frames.append(giant_ok)
            want.append(CODE_BASE + 14)                  # untagged IPv6 + ICMPv6
        else:
            coded(int(rng.choice(codes)))
    for _ in range(37):
        coded(int(rng.choice(codes)))
    return frames, np.array(want, np.int64)


ETH_LENS = (14, 18, 22)


def window_families(rng):
    """{"A" | "B" | "C": frames}: see tests/test_gpu_paths.py case 8.
    A: IPv6 + a Hop-by-Hop header of 0-80 B + TCP / UDP / ICMPv6 (L4 at
    54-142). B: an outer IPv4 of IHL 5-15 or an outer IPv6, an inner IPv4 /
    IPv6 / IPv6 + 16-B Destination Options, then TCP / UDP / ICMP. C: as B
    under an outer IPv6 with a Hop-by-Hop header of 16-56 B, which puts the
    inner IP header on and past the window end."""
    inners = (("v4", 5), ("v6", []), ("v6", [(60, 16)]))
    icmp = lambda lv: "icmpv4" if lv[0] == "v4" else "icmpv6"
    a, b, c = [], [], []
    for eth_len in ETH_LENS:
        for e in range(0, 88, 8):
            for l4 in ("tcp", "udp", "icmpv6"):
                a.append(stack(rng, eth_len, [("v6", [(0, e)] if e else [])], l4, min_payload=24))
        outers = [("v4", ihl) for ihl in range(5, 16, 2)] + [("v6", [])]
        for outer in outers:
            for inner in inners:
                for l4 in ("tcp", "udp", icmp(inner)):
                    b.append(stack(rng, eth_len, [outer, inner], l4, min_payload=24))
        for h in range(16, 64, 8):
            for inner in inners:
                for l4 in ("tcp", "udp", icmp(inner)):
                    c.append(stack(rng, eth_len, [("v6", [(0, h)]), inner], l4, min_payload=24))
    return {"A": a, "B": b, "C": c}


def bare_stack(rng, eth_len, levels, l4):
    """stack() without payload: the frame ends at the last byte of its L4
    header (8 B of UDP / ICMP), for l4 "none" at the last byte of its
    innermost IP header. The reference rejects a frame under 64 B
    (ethernet.rs: the minimum frame size), so a shorter stack gets the
    payload that brings it to 64 B, the smallest it accepts."""
    size = max(64, eth_len + L4_MIN[l4] + sum(
        lv[1] * 4 if lv[0] == "v4" else 40 + sum(s for _, s in lv[1]) for lv in levels))
    f = ethernet(rng, eth_len, 0x0800 if levels[0][0] == "v4" else 0x86DD)
    left = size - eth_len
    for k, lv in enumerate(levels):
        nxt = L4_PROTO[l4] if k + 1 == len(levels) else (4 if levels[k + 1][0] == "v4" else 41)
        if lv[0] == "v4":
            left -= lv[1] * 4
            f += ipv4(rng, lv[1], nxt, left)
        else:
            chain = lv[1]
            left -= 40
            f += ipv6(rng, chain[0][0] if chain else nxt, left)
            for j, (_, s) in enumerate(chain):
                f += options(rng, chain[j + 1][0] if j + 1 < len(chain) else nxt, s)
                left -= s
    f += l4_segment(rng, l4, left)
    assert len(f) == size and (left == L4_MIN[l4] or size == 64)
    return repair(bytes(f))


def short_tail_families(rng):
    """{"A" | "B" | "C": frames}: the stacks of window_families() as
    bare_stack() frames, so that every frame is shorter than the bytes a
    column reader asks for (l4 + 20, inner + 40 or l3 + 40) and its header
    window ends with the frame. L4: UDP and ICMP (8 B, where a TCP header
    would have 20), and "none" where the innermost IP header is an IPv4 one:
    that frame ends 20 B into the 40 a reader asks for (behind an IPv6 header
    without L4 nothing is missing, so those stacks are left out)."""
    inners = (("v4", 5), ("v6", []), ("v6", [(60, 16)]))
    kinds = lambda lv: ("udp", "icmpv4", "none") if lv[0] == "v4" else ("udp", "icmpv6")
    a, b, c = [], [], []
    for eth_len in ETH_LENS:
        for e in range(0, 88, 8):
            for l4 in ("udp", "icmpv6"):
                a.append(bare_stack(rng, eth_len, [("v6", [(0, e)] if e else [])], l4))
        outers = [("v4", ihl) for ihl in range(5, 16, 2)] + [("v6", [])]
        for outer in outers:
            for inner in inners:
                for l4 in kinds(inner):
                    b.append(bare_stack(rng, eth_len, [outer, inner], l4))
        for h in range(16, 64, 8):
            for inner in inners:
                for l4 in kinds(inner):
                    c.append(bare_stack(rng, eth_len, [("v6", [(0, h)]), inner], l4))
    return {"A": a, "B": b, "C": c}


def with_filler(arena, offs, lens, fill):
    """A copy of the arena with every byte that belongs to no frame set to `fill`."""
    own = np.zeros(len(arena), bool)
    for o, n in zip(offs, lens):
        own[int(o):int(o) + int(n)] = True
    out = arena.copy()
    out[~own] = fill
    return out


def place_aligned(frames):
    """Each frame at each start alignment s = 0..15 (start = the next multiple
    of 16, plus s). Returns (arena, offs, lens, frame index of each
    descriptor); the arena ends at the last frame's last byte."""
    offs, lens, idx, pos = [], [], [], 0
    for s in range(16):
        for k, f in enumerate(frames):
            at = (pos + 15) // 16 * 16 + s
            offs.append(at)
            lens.append(len(f))
            idx.append(k)
            pos = at + len(f)
    arena = np.zeros(pos, np.uint8)
    for o, k in zip(offs, idx):
        arena[o:o + len(frames[k])] = np.frombuffer(frames[k], np.uint8)
    return arena, np.array(offs, np.uint64), np.array(lens, np.uint32), np.array(idx, np.int64)
