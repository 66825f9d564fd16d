"""Frames whose L4 word sum sits on a multiple of 2^32 (test infrastructure).

The reference adds 16-bit words into a u32 that wraps (checksum.rs:5-29), and
2^32 = 1 (mod 65535): every wrap shifts the folded sum by one, and a wrapped
sum of exactly 0 folds to 0. Only an L4 slice of ZP_REWRITE_EXACT_L4_BYTES
(131,037) or more can get there, i.e. TCP or ICMPv6 in an IPv6 jumbogram
(parser.rs never checks the IPv6 payload length; the UDP length check and the
IPv4 total-length check exclude the rest).

wrap_frame builds Ethernet / IPv6 / {TCP, ICMPv6} whose L4 slice plus
pseudo-header, with the checksum field zero, sums to a requested exact
integer S0: the payload is 0xFF throughout and whole words are lowered from
the tail until the sum fits. Everything here is plain integer arithmetic,
independent of the oracle; tests/test_wrap_boundary.py checks each fixture
against the oracle on the CPU before any GPU test uses it.
"""
import functools

import numpy as np

MAC_D, MAC_S = bytes([0x04, 0xb4, 0xfe, 0x9a, 0x81, 0xc7]), bytes([0x34, 0x97, 0xf6, 0x94, 0x02, 0x0f])
SRC6 = bytes([0x20, 0x01, 0x0d, 0xb8, 0x85, 0xa3, 0, 0, 0, 0, 0x8a, 0x2e, 0x03, 0x70, 0x73, 0x34])
DST6 = bytes([0xfe, 0x80, 0, 0, 0, 0, 0, 0, 0x02, 0x02, 0xb3, 0xff, 0xfe, 0x1e, 0x83, 0x29])
OUT_S6 = bytes([0x20, 0x01, 0x0d, 0xb8] + list(range(1, 13)))
OUT_D6 = bytes([0xfd] + list(range(100, 115)))
TCP, ICMPV6 = 6, 58
W = 1 << 32


def fold(s):
    """checksum.rs:22-28 of the u32 sum s -> the stored checksum."""
    assert 0 <= s < W
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return ~s & 0xFFFF


def stored_for(s0):
    """The checksum the reference's writers store over a slice whose exact
    sum (pseudo-header included, field zero) is s0: the sum wraps first."""
    return fold(s0 % W)


def accepts(total):
    """verify_internet_checksum (checksum.rs:33-35) of the exact total."""
    return fold(total % W) == 0


class WrapFrame:
    """frame: bytes; l4: L4 offset; ck: checksum field offset; ip: offset of
    the IPv6 header whose addresses the pseudo-header takes; proto."""

    def __init__(self, frame, l4, ck, ip, proto):
        self.frame, self.l4, self.ck, self.ip, self.proto = frame, l4, ck, ip, proto

    def s0(self, frame=None):
        """Exact integer sum of pseudo-header + L4 words, checksum field zero."""
        return exact_sum(self.frame if frame is None else frame, self.l4, self.ck, self.ip,
                         self.proto)

    def stored(self, frame=None):
        f = self.frame if frame is None else frame
        return (f[self.ck] << 8) | f[self.ck + 1]

    def total(self, frame=None):
        return self.s0(frame) + self.stored(frame)

    def with_checksum(self, c):
        f = bytearray(self.frame)
        f[self.ck:self.ck + 2] = c.to_bytes(2, "big")
        return WrapFrame(bytes(f), self.l4, self.ck, self.ip, self.proto)


def exact_sum(frame, l4, ck, ip, proto):
    a = np.frombuffer(frame, np.uint8)
    seg = a[l4:]
    n = len(seg) & ~1
    s = int(seg[:n].view(">u2").astype(np.int64).sum()) if l4 % 2 == 0 else \
        int((seg[:n:2].astype(np.int64) << 8).sum() + seg[1:n:2].astype(np.int64).sum())
    if len(seg) & 1:
        s += int(seg[-1]) << 8
    s -= (frame[ck] << 8) | frame[ck + 1]
    adr = a[ip + 8:ip + 40].astype(np.int64)
    return s + int((adr[0::2] << 8).sum() + adr[1::2].sum()) + proto + len(seg)


def _ip6(nh, plen, src, dst):
    return bytes([0x60, 0, 0, 0]) + (plen & 0xFFFF).to_bytes(2, "big") + bytes([nh, 64]) + src + dst


@functools.lru_cache(maxsize=None)
def wrap_frame(proto, s0, l4_len, sp=1, dp=2, tags=(), tunnel=False):
    """Ethernet (+ VLAN tags) / IPv6 / L4 of l4_len bytes, exact sum s0, the
    reference's checksum stored. tunnel: an outer IPv6 in front, and an 8-B
    Destination Options header between the inner IPv6 header and the L4."""
    eth = MAC_D + MAC_S
    for tpid, tci in tags:
        eth += tpid.to_bytes(2, "big") + tci.to_bytes(2, "big")
    eth += b"\x86\xdd"
    if proto == TCP:                      # 20-B header, PSH | ACK, window 0x2000
        hdr = sp.to_bytes(2, "big") + dp.to_bytes(2, "big") + bytes(8) + b"\x50\x18\x20\x00" + \
            bytes(4)
        ckx = 16
    else:                                 # echo request, identifier and sequence 0
        hdr = b"\x80\0\0\0" + bytes(4)
        ckx = 2
    ip = len(eth)
    if tunnel:
        head = eth + _ip6(41, 48 + l4_len, OUT_S6, OUT_D6)
        ip = len(head)
        head += _ip6(60, 8 + l4_len, SRC6, DST6) + bytes([proto, 0, 1, 4, 0, 0, 0, 0])
    else:
        head = eth + _ip6(proto, l4_len, SRC6, DST6)
    l4 = len(head)
    f = bytearray(head + hdr + b"\xff" * (l4_len - len(hdr)))
    wf = WrapFrame(bytes(f), l4, l4 + ckx, ip, proto)
    over = wf.s0() - s0
    assert over >= 0, ("an all-0xFF slice of this length sums below s0", wf.s0(), s0)
    x = l4 + (l4_len & ~1) - 2            # the last whole word of the slice
    while over:
        assert x >= l4 + len(hdr), "s0 is out of the payload's reach"
        dec = min(over, 0xFFFF)
        f[x:x + 2] = (0xFFFF - dec).to_bytes(2, "big")
        over -= dec
        x -= 2
    wf = WrapFrame(bytes(f), l4, l4 + ckx, ip, proto)
    assert wf.s0() == s0
    return wf.with_checksum(stored_for(s0))


# ---- parse fixtures --------------------------------------------------------
# name -> (frame, exact total with the stored checksum, accepted). An odd
# length puts the last payload byte into the high half of a padded word.
L_ONE, L_TWO = 131120, 262400             # slices that can wrap once / twice


@functools.lru_cache(maxsize=None)
def parse_fixtures():
    out = {}

    def add(name, wf, total, ok):
        assert wf.total() == total and accepts(total) == ok, name
        out[name] = (wf.frame, total, ok)

    for tag, n in (("", L_ONE), ("_odd", L_ONE + 1)):
        a = wrap_frame(TCP, W - 0x100, n)              # stored 0x00FF
        add("ffffffff" + tag, a, W - 1, True)          # no wrap, valid
        add("ffffffff_bad" + tag, a.with_checksum(0x00FE), W - 2, False)
        b = wrap_frame(ICMPV6, W + 0x8000, n)          # stored 0x7FFF
        add("wrap_ffff" + tag, b, W + 0xFFFF, True)    # valid only under wrap arithmetic
        add("wrap_ffff_bad" + tag, b.with_checksum(0x7FFF ^ 0x0100), W + 0xFFFF - 0x100, False)
    a = wrap_frame(TCP, W - 0x100, L_ONE)
    add("two32", a.with_checksum(0x0100), W, False)    # wrapped sum 0 (checksum.rs:28)
    b = wrap_frame(ICMPV6, W + 0x8000, L_ONE)
    add("wrap_fffe", b.with_checksum(0x7FFE), W + 0xFFFE, False)   # = 0 (mod 65535), invalid
    c = wrap_frame(TCP, 2 * W + 0x1234, L_TWO)         # two wraps: stored ~0x1234
    add("twice", c, 2 * W + 0xFFFF, True)
    bad = c.with_checksum(c.stored() ^ 1)
    add("twice_bad", bad, bad.total(), False)
    return out


# ---- rewrite fixtures ------------------------------------------------------
# name -> (WrapFrame, {column: value written at that frame} or "identity" (all
#          14 columns as extracted), wrap counts (before, after) of the exact
#          sum with the field zero).
VLAN = ((0x8100, 0x2005),)


def _bump(addr, by):
    """addr with its last 16-bit word raised by `by`."""
    v = ((addr[14] << 8) | addr[15]) + by
    assert 0 <= v <= 0xFFFF
    return addr[:14] + v.to_bytes(2, "big")


@functools.lru_cache(maxsize=None)
def rewrite_fixtures():
    w1 = wrap_frame(TCP, W - 0x100, L_ONE)
    w2 = wrap_frame(TCP, W + 0x80, L_ONE, sp=0x0400)
    w3 = wrap_frame(TCP, W + 0x10000, L_ONE)
    w5 = wrap_frame(ICMPV6, W - 0x100, L_ONE)
    w6 = wrap_frame(TCP, W - 0x100, L_ONE, tags=VLAN)
    w8 = wrap_frame(TCP, W - 0x100, L_ONE, tunnel=True)
    return {
        "W1": (w1, {"src_port": 0x0200, "dest_port": 2}, (0, 1)),
        "W1_ffff": (w1, {"src_port": 0xFFFF}, (0, 1)),
        "W1_below": (w1, {"src_port": 0x00F0}, (0, 0)),
        "W2": (w2, {"src_port": 0x0100, "dest_port": 1}, (1, 0)),
        "W3": (w3, {"src_port": 2}, (1, 1)),
        "W4": (w1, {"src_addr": _bump(SRC6, 0x200)}, (0, 1)),
        "W5": (w5, {"dest_addr": _bump(DST6, 0x200)}, (0, 1)),
        "W6": (w6, {"src_port": 0x0200, "dest_port": 2}, (0, 1)),
        "W7": (w1, "identity", (0, 0)),
        "W8_tunnel": (w8, {"src_port": 0x0200, "tcp_seq": 7}, (0, 1)),
    }
