"""Batched header rewrite (zp_rewrite_columns_device, columns.rewrite).

CPU: the writable-column table of the C ABI, the argument checks that need no
device, and tests/rewrite_ref.py pinned to the reference's writers through the
builder oracle: rewrite_ref(build(A), A -> B) == build(B).
GPU: the kernel's bytes equal rewrite_ref (full checksum recomputes), the
oracle re-parses the output to the same records, and the oracle's columns of
the output hold the written values where they apply and the old ones elsewhere.
"""
import ctypes
import random

import numpy as np
import pytest

import oracle as orc
from fuzzfix import repair
from rewrite_ref import NAT, WRITABLE, rewrite_batch_ref, rewrite_ref

SPEC = {name: (dt, w) for name, dt, w in orc.COLUMN_SPEC}


# ---- CPU: ABI table and argument checks ------------------------------------

def test_writable_table(zp):
    lib = zp._lib.hip()
    names = [c[0] for c in orc.COLUMN_SPEC]
    for k, name in enumerate(names):
        assert lib.zp_col_writable(k) == int(name in WRITABLE), name
    assert lib.zp_col_writable(-1) == 0 and lib.zp_col_writable(len(names)) == 0
    assert tuple(zp.columns.WRITABLE) == WRITABLE and len(WRITABLE) == 14
    assert lib.zp_abi_version() == 6


def test_rewrite_refusals_touch_no_device(zp):
    """A non-writable column pointer is refused before any launch and the
    message names the column; n == 0 returns 0 (neither needs a device)."""
    lib = zp._lib.hip()
    names = [c[0] for c in orc.COLUMN_SPEC]
    for bad in ("ethertype", "inner_src_addr", "l4_checksum", "tcp_flags", "ip_len"):
        ptrs = (ctypes.c_void_p * len(names))()
        ptrs[names.index("ttl")] = 64                    # never dereferenced
        ptrs[names.index(bad)] = 64
        rc = lib.zp_rewrite_columns_device(64, 64, 64, 64, 10, ptrs, None)
        assert rc < 0
        assert bad.upper() in lib.zp_last_error().decode()
    ptrs = (ctypes.c_void_p * len(names))()
    ptrs[names.index("ttl")] = 64
    assert lib.zp_rewrite_columns_device(64, 64, 64, 64, 0, ptrs, None) == 0
    assert lib.zp_rewrite_columns_device(None, None, None, None, 0, None, None) == 0


# ---- CPU: rewrite_ref against the reference's builder ----------------------

M = [[0x34, 0x97, 0xf6, 0x94, 0x02, 0x0f], [0x04, 0xb4, 0xfe, 0x9a, 0x81, 0xc7],
     [0x02, 0x11, 0x22, 0x33, 0x44, 0x55], [0x0a, 0xbb, 0xcc, 0xdd, 0xee, 0xff]]
IP4 = [[192, 168, 1, 1], [192, 168, 1, 2], [10, 9, 8, 7], [172, 16, 254, 3]]
IP6 = [[0x20, 0x01, 0x0d, 0xb8, 0x85, 0xa3, 0, 0, 0, 0, 0x8a, 0x2e, 0x03, 0x70, 0x73, 0x34],
       [0xfe, 0x80, 0, 0, 0, 0, 0, 0, 0x02, 0x02, 0xb3, 0xff, 0xfe, 0x1e, 0x83, 0x29],
       [0x20, 0x01, 0x0d, 0xb8] + list(range(1, 13)), [0xfd] + list(range(100, 115))]
# field values A / B; A's IPv4 / TCP values are the tcp_in_ipv4_in_ethernet
# golden vector's (builder.rs:1097-1101)
VA = dict(smac=M[0], dmac=M[1], s4=IP4[0], d4=IP4[1], s6=IP6[0], d6=IP6[1], dscp=99, ecn=123,
          id=54321, ttl=123, sp=99, dp=11, seq=123, ack=321, win=4321, tci=200, tci2=100, tc=5,
          fl=4)
VB = dict(smac=M[2], dmac=M[3], s4=IP4[2], d4=IP4[3], s6=IP6[2], d6=IP6[3], dscp=17, ecn=2,
          id=777, ttl=9, sp=40000, dp=443, seq=0xDEADBEEF, ack=0x01020304, win=65535, tci=0x3abc,
          tci2=0x0fff, tc=0xb7, fl=0xabcde)


def _chain(zp, stack, v):
    """The builder chain of `stack` with field values v -> (chain, buffer
    length, hand-made oracle-style record). The golden vectors do not parse
    (version 99, total_length 12345), so the record is stated here."""
    C = zp.builder.Chain()
    eth, hl = ("plain", 14)
    if stack == "vlan":
        eth, hl = "vlan", 18
    elif stack == "qinq":
        eth, hl = "qinq", 22
    l3 = "v6" if stack in ("tcp6", "udp6", "icmpv6", "ipip") else "v4"
    et = 0x86DD if l3 == "v6" else 0x0800
    if eth == "plain":
        C.ethernet(v["smac"], v["dmac"], et)
    elif eth == "vlan":
        C.ethernet_vlan(v["smac"], v["dmac"], et, v["tci"])
    else:
        C.ethernet_qinq(v["smac"], v["dmac"], et, v["tci"], v["tci2"])
    l4 = {"tcp4": "tcp", "udp4": "udp", "icmpv4": "icmpv4", "tcp6": "tcp", "udp6": "udp",
          "icmpv6": "icmpv6", "vlan": "tcp", "qinq": "udp", "ipip": "tcp"}[stack]
    proto = {"tcp": 6, "udp": 17, "icmpv4": 1, "icmpv6": 58}[l4]
    flags = 1 | {"tcp": 64, "udp": 128, "icmpv4": 256, "icmpv6": 512}[l4]
    pos, inner_off = hl, 0
    if l3 == "v4":
        ver = 99 if stack == "tcp4" else 4             # the golden vector's version
        C.ipv4(ver, 5, v["dscp"], v["ecn"], 12345, v["id"], 99, 12345, v["ttl"], proto,
               v["s4"], v["d4"])
        flags |= 4
        pos += 20
        src, dst = v["s4"], v["d4"]
    else:
        C.ipv6(6, v["tc"], v["fl"], 31, 4 if stack == "ipip" else proto, v["ttl"], v["s6"],
               v["d6"])
        flags |= 8
        pos += 40
        src, dst = v["s6"], v["d6"]
    if stack == "ipip":                                # the inner header is not writable
        src, dst = IP4[1], IP4[0]
        C.ipv4(4, 5, 0, 0, 150, 0, 0, 0, 64, proto, src, dst)
        flags |= 16
        inner_off = pos
        pos += 20
    pay = list(range(1, 11))
    if l4 == "tcp":
        C.tcp(src, v["sp"], dst, v["dp"], v["seq"], v["ack"], 11 if stack == "tcp4" else 5, 99,
              99, v["win"], 1234, None if stack == "tcp4" else pay)
    elif l4 == "udp":
        C.udp(src, v["sp"], dst, v["dp"], 4321, pay)
    elif l4 == "icmpv4":
        C.icmpv4(8, 0, pay)
    else:
        C.icmpv6(src, dst, 128, 0, pay)
    n = 54 if stack == "tcp4" else 120
    rec = np.zeros(1, orc.RECORD_DTYPE)[0]
    rec["flags"], rec["eth_len"], rec["l4_off"], rec["inner_off"] = flags, hl, pos, inner_off
    rec["final_nh"] = proto if l3 == "v6" and stack != "ipip" else (4 if stack == "ipip" else 0)
    return C, n, rec


def _writes(v, v6):
    pad = lambda a: bytes(a) + bytes(16 - len(a))
    return dict(dest_mac=bytes(v["dmac"]), src_mac=bytes(v["smac"]), vlan_tci=v["tci"],
                vlan_inner_tci=v["tci2"], src_addr=pad(v["s6"] if v6 else v["s4"]),
                dest_addr=pad(v["d6"] if v6 else v["d4"]), ttl=v["ttl"],
                tos=v["tc"] if v6 else ((v["dscp"] << 2) | (v["ecn"] & 3)) & 0xFF,
                ip_id=v["fl"] if v6 else v["id"], src_port=v["sp"], dest_port=v["dp"],
                tcp_seq=v["seq"], tcp_ack=v["ack"], tcp_window=v["win"])


STACKS = ["tcp4", "udp4", "icmpv4", "tcp6", "udp6", "icmpv6", "vlan", "qinq", "ipip"]


def test_rewrite_ref_equals_builder(zp, golden):
    from test_builder import run_oracle
    assert set(WRITABLE) == set(zp.columns.WRITABLE)   # the restatement covers the module's set
    vec = {v["name"]: bytes.fromhex(v["bytes"]) for v in golden["builder_vectors"]}
    seen = set()
    for stack in STACKS:
        ca, n, rec = _chain(zp, stack, VA)
        cb, _, _ = _chain(zp, stack, VB)
        _, arena, offs, lens, res, _ = run_oracle(zp, [ca, cb], [n, n])
        assert (res["err"] == 0).all(), (stack, res)
        fa = arena[int(offs[0]):int(offs[0]) + n].tobytes()
        fb = arena[int(offs[1]):int(offs[1]) + n].tobytes()
        if stack == "tcp4":
            assert fa == vec["tcp_in_ipv4_in_ethernet"]
        ext = np.zeros(2, orc.EXT_DTYPE)
        got, applied = rewrite_ref(fa, rec, ext, _writes(VB, bool(int(rec["flags"]) & 8)))
        assert got == fb, (stack, got.hex(), fb.hex())
        assert all(applied.values()), (stack, applied)  # A and B differ in every applied field
        seen |= set(applied)
        # and back: B -> A
        back, _ = rewrite_ref(fb, rec, ext, _writes(VA, bool(int(rec["flags"]) & 8)))
        assert back == fa, stack
    assert seen == set(WRITABLE)


# ---- GPU -------------------------------------------------------------------

def random_cols(rng, n, names):
    cols = {}
    for name in names:
        dt, w = SPEC[name]
        hi = np.iinfo(dt).max
        cols[name] = rng.integers(0, hi, (n, w) if w > 1 else (n,), dtype=dt, endpoint=True)
    return cols


GUARD = 0xA5


def as_extracted(name, wr, orec):
    """A written column as the extract reads it back where it applied."""
    if name in ("src_addr", "dest_addr"):               # IPv4: bytes 0-3, the rest reads 0
        wr = wr.copy()
        wr[(orec["flags"] & 4) != 0, 4:] = 0
    elif name == "ip_id":                               # 16 bits of IPv4 id, 20 of flow label
        wr = np.where((orec["flags"] & 4) != 0, wr & 0xFFFF, wr & 0xFFFFF).astype(wr.dtype)
    return wr


def frames_at(offs, lens, where):
    """The descriptor index that owns each arena offset in `where` (-1: none,
    a byte between or outside the frames), for descriptors in any order."""
    offs, lens = np.asarray(offs).astype(np.int64), np.asarray(lens).astype(np.int64)
    order = np.argsort(offs, kind="stable")
    j = np.searchsorted(offs[order], where, side="right") - 1
    own = order[np.maximum(j, 0)]
    return np.where((j >= 0) & (np.asarray(where) < offs[own] + lens[own]), own, -1)


def run_rewrite(zp, arena, offs, lens, cols, base=0, stream=None, guard=64):
    """Parses and rewrites on the GPU; checks (a) bytes == rewrite_ref, (b) the
    oracle re-parses the output to the same packed records, (c) the oracle's
    columns of the output. Returns (output arena, changed masks, oracle records).
    base: leading bytes in front of the arena view (shifts its alignment);
    guard: bytes behind it (0: the arena ends on the allocation's last byte).
    Both hold GUARD before and must hold it afterwards."""
    import torch
    d = torch.device("cuda:0")
    whole = torch.full((base + len(arena) + guard,), GUARD, dtype=torch.uint8, device=d)
    a = whole[base:base + len(arena)]
    a.copy_(torch.from_numpy(arena))
    o = torch.from_numpy(offs.astype(np.int64)).to(d)
    l_ = torch.from_numpy(lens.astype(np.int32)).to(d)
    recs, _ = zp.batch.parse_batch(a, o, l_)
    tc = {k: torch.from_numpy(np.ascontiguousarray(v)).to(d) for k, v in cols.items()}
    if stream is None:
        zp.columns.rewrite(a, o, l_, recs, tc)
    else:
        stream.wait_stream(torch.cuda.current_stream(d))
        with torch.cuda.stream(stream):
            zp.columns.rewrite(a, o, l_, recs, tc, stream=stream.cuda_stream)
        stream.synchronize()
    torch.cuda.synchronize()
    got = a.cpu().numpy()
    orec, oext = orc.parse_batch(arena, offs, lens)
    packed = orc.pack(orec, oext)
    assert recs.cpu().numpy().tobytes() == packed.tobytes()
    want, changed, applied = rewrite_batch_ref(arena, offs, lens, orec, oext, cols)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, ("bytes differ from rewrite_ref at arena offsets", bad[:8],
                           "frames", frames_at(offs, lens, bad[:8]))                      # (a)
    assert (whole[:base] == GUARD).all() and (whole[base + len(arena):] == GUARD).all()
    nrec, next_ = orc.parse_batch(got, offs, lens)
    assert orc.pack(nrec, next_).tobytes() == packed.tobytes()                            # (b)
    old = orc.columns(arena, offs, lens, orec)
    new = orc.columns(got, offs, lens, nrec)
    for name, _, _ in orc.COLUMN_SPEC:                                                     # (c)
        if name in cols:
            m = applied[name]
            wr = as_extracted(name, cols[name], orec)
            assert np.array_equal(new[name][m], wr[m]), name
            assert np.array_equal(new[name][~m], old[name][~m]), name
        elif name != "l4_checksum":
            assert np.array_equal(new[name], old[name]), name
    return got, changed, orec


@pytest.mark.gpu
def test_gpu_rewrite_corpus(zp, golden):
    from test_columns import frames_corpus, pack
    arena, offs, lens = pack(frames_corpus(zp, golden, 2500, seed=11))
    cols = random_cols(np.random.default_rng(5), len(offs), WRITABLE)
    got, changed, orec = run_rewrite(zp, arena, offs, lens, cols)
    rej = orec["err"] != 0
    assert rej.any() and (~rej).any()
    for i in np.nonzero(rej)[0]:                        # rejected frames: untouched
        o, l_ = int(offs[i]), int(lens[i])
        assert got[o:o + l_].tobytes() == arena[o:o + l_].tobytes(), i
    assert all(changed[k].any() for k in WRITABLE)


@pytest.mark.gpu
@pytest.mark.parametrize("names", [WRITABLE, NAT], ids=["all14", "nat"])
@pytest.mark.parametrize("cfg", ["c3", "c4", "c5", "c6"])
def test_gpu_rewrite_generated(zp, cfg, names):
    """n = 4099: a partial last workgroup; frames packed back to back, so every
    byte alignment occurs. Every column whose reader some frame of the config
    has must have been applied with a changed value (c3 is plain IPv4 without
    tags: its VLAN columns apply nowhere); c5 / c6 have every reader."""
    arena, offs, lens = zp.batch.generate_host(cfg, 4099, first=77)
    cols = random_cols(np.random.default_rng(int(cfg[1]) + len(names)), len(offs), names)
    _, changed, orec = run_rewrite(zp, arena, offs, lens, cols)
    fl, hl = orec["flags"], orec["eth_len"]
    present = {"vlan_tci": (hl >= 18).any(), "vlan_inner_tci": (hl == 22).any(),
               "tcp_seq": (fl & 64).any(), "tcp_ack": (fl & 64).any(),
               "tcp_window": (fl & 64).any()}
    for k in names:
        assert changed[k].any() == bool(present.get(k, True)), (cfg, k)
        if cfg in ("c5", "c6"):
            assert changed[k].any(), (cfg, k)
    if cfg == "c4":
        assert (orec["l4_off"] + 20 > 112).any()        # L4 headers past the staged window


@pytest.mark.gpu
def test_gpu_rewrite_single_columns(zp):
    """Each column of an adjacent pair alone (the kernel writes the MACs, the
    addresses and the TCP ports / sequence / acknowledgment numbers in one run
    when all of a run's columns are given, and field by field otherwise)."""
    arena, offs, lens = zp.batch.generate_host("c5", 700, first=21)
    for k, names in enumerate([("dest_mac",), ("src_mac",), ("src_addr",), ("dest_addr",),
                               ("src_port",), ("dest_port",), ("tcp_seq", "src_port"),
                               ("tcp_ack", "dest_port", "src_port"),
                               ("src_port", "dest_port", "tcp_seq")]):
        cols = random_cols(np.random.default_rng(40 + k), len(offs), names)
        _, changed, _ = run_rewrite(zp, arena, offs, lens, cols)
        assert all(changed[n].any() for n in names), names


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [1, 2, 3])
def test_gpu_rewrite_neighbours(zp, shift):
    """64-B frames back to back behind an arena view shifted by 1-3 bytes:
    every frame's first and last bytes share a dword with a neighbour, and the
    MAC / port writes of frame i must leave frames i +- 1 as rewrite_ref says."""
    arena, offs, lens = zp.batch.generate_host("c2", 1000, first=5)
    assert (lens == 64).all() and (np.diff(offs.astype(np.int64)) == 64).all()
    cols = random_cols(np.random.default_rng(shift), 1000,
                       ("dest_mac", "src_mac", "src_port", "dest_port"))
    _, changed, _ = run_rewrite(zp, arena, offs, lens, cols, base=shift)
    assert all(c.sum() > 990 for c in changed.values())


def _eth(et, tags=()):
    b = bytes(M[1]) + bytes(M[0])
    for tpid, tci in tags:
        b += tpid.to_bytes(2, "big") + tci.to_bytes(2, "big")
    return b + et.to_bytes(2, "big")


def _ip4(proto, body, ihl=5, src=IP4[0], dst=IP4[1], ttl=64):
    h = bytearray(ihl * 4)
    h[0] = 0x40 | ihl
    h[2:4] = (ihl * 4 + len(body)).to_bytes(2, "big")
    h[4:6] = b"\x12\x34"
    h[8], h[9] = ttl, proto
    h[12:16], h[16:20] = bytes(src), bytes(dst)
    for k in range(20, ihl * 4):
        h[k] = 1                                        # NOP options
    return bytes(h) + body


def _ip6(nh, body, src=IP6[0], dst=IP6[1]):
    return bytes([0x60, 0, 0, 0]) + len(body).to_bytes(2, "big") + bytes([nh, 64]) + \
        bytes(src) + bytes(dst) + body


def _udp(sp, dp, pay):
    return sp.to_bytes(2, "big") + dp.to_bytes(2, "big") + (8 + len(pay)).to_bytes(2, "big") + \
        b"\0\0" + pay


def _tcp(sp, dp, pay):
    return sp.to_bytes(2, "big") + dp.to_bytes(2, "big") + bytes(8) + b"\x50\x18\x20\x00" + \
        bytes(4) + pay


def _udp_ffff(sp):
    """Ethernet / IPv4 / UDP whose canonical checksum is 0x0000, stored as
    0xFFFF (still valid: the sum verifies either way)."""
    f = bytearray(repair(_eth(0x0800) + _ip4(17, _udp(sp, 53, bytes(30)))))
    c = (f[40] << 8) | f[41]                            # checksum with payload word 0 = 0
    f[42:44] = c.to_bytes(2, "big")                     # ... so this word makes the sum 0xFFFF
    assert repair(bytes(f))[40:42] == b"\0\0"
    f[40:42] = b"\xff\xff"
    return bytes(f)


EDGE = ["udp_ffff", "udp_ffff_t0", "icmp4_v4", "icmp4_v6", "icmp6_v4", "tunnel", "ihl7", "same"]


def edge_frames():
    pay = bytes(range(40))
    fr = {
        "udp_ffff": _udp_ffff(0x1234),
        "udp_ffff_t0": _udp_ffff(0xFFFF),
        "icmp4_v4": repair(_eth(0x0800) + _ip4(1, b"\x08\0\0\0" + pay)),
        "icmp4_v6": repair(_eth(0x86DD) + _ip6(1, b"\x08\0\0\0" + pay)),
        "icmp6_v4": repair(_eth(0x0800) + _ip4(58, b"\x80\0\0\0" + pay)),
        "tunnel": repair(_eth(0x0800) + _ip4(4, _ip4(17, _udp(7, 9, pay), src=IP4[2], dst=IP4[3]))),
        "ihl7": repair(_eth(0x0800) + _ip4(6, _tcp(80, 8080, pay), ihl=7)),
        "same": repair(_eth(0x0800, [(0x8100, 5)]) + _ip4(6, _tcp(1, 2, pay))),
    }
    return [fr[k] for k in EDGE]


@pytest.mark.gpu
def test_gpu_rewrite_checksum_edges(zp):
    from test_columns import pack
    frames = edge_frames()
    arena, offs, lens = pack(frames)
    orec, oext = orc.parse_batch(arena, offs, lens)
    assert (orec["err"] == 0).all(), orec["err"]
    old = orc.columns(arena, offs, lens, orec)
    ix = {k: i for i, k in enumerate(EDGE)}
    fr = lambda a, k: a[int(offs[ix[k]]):int(offs[ix[k]]) + int(lens[ix[k]])].tobytes()

    # identity over all 14 columns: nothing changes, the stored 0xFFFF stays
    got, changed, _ = run_rewrite(zp, arena, offs, lens, {k: old[k].copy() for k in WRITABLE})
    assert np.array_equal(got, arena) and not any(c.any() for c in changed.values())
    # TTL written to the same value, alone
    got, _, _ = run_rewrite(zp, arena, offs, lens, {"ttl": old["ttl"].copy()})
    assert np.array_equal(got, arena)

    cols = {k: old[k].copy() for k in NAT}
    cols["dest_port"][ix["udp_ffff"]] = 5353
    cols["src_port"][ix["udp_ffff_t0"]] = 0             # 0xFFFF -> 0: T = 0
    for k in ("icmp4_v4", "icmp4_v6", "icmp6_v4", "tunnel"):
        cols["src_addr"][ix[k], :4] = [11, 22, 33, 44]
    cols["dest_addr"][ix["ihl7"], :4] = [9, 9, 9, 9]
    cols["ttl"][ix["ihl7"]] = 1
    got, changed, _ = run_rewrite(zp, arena, offs, lens, cols)
    # the T = 0 case and its neighbour give the full-recompute value
    for k in ("udp_ffff", "udp_ffff_t0"):
        f = fr(got, k)
        assert f == repair(f) and f != fr(arena, k), k
    assert fr(got, "udp_ffff_t0")[40:42] == b"\0\0" and fr(got, "udp_ffff_t0")[34:36] == b"\0\0"
    ck = lambda a, k, x: fr(a, k)[x:x + 2]
    # ICMPv4 under IPv4: no pseudo-header; the header checksum moves
    assert ck(got, "icmp4_v4", 36) == ck(arena, "icmp4_v4", 36)
    assert ck(got, "icmp4_v4", 24) != ck(arena, "icmp4_v4", 24)
    # ICMPv4 under IPv6 and ICMPv6 under IPv4: the L4 checksum covers the addresses
    assert ck(got, "icmp4_v6", 56) != ck(arena, "icmp4_v6", 56)
    assert ck(got, "icmp6_v4", 36) != ck(arena, "icmp6_v4", 36)
    # a tunnel: the outer address is in no L4 pseudo-header
    assert ck(got, "tunnel", 60) == ck(arena, "tunnel", 60)
    assert ck(got, "tunnel", 24) != ck(arena, "tunnel", 24)
    # IPv4 options (IHL 7): the TCP header starts at 42
    assert fr(got, "ihl7") == repair(fr(got, "ihl7")) and fr(got, "ihl7")[22] == 1
    assert fr(got, "same") == fr(arena, "same")
    for k in EDGE:                                      # full recomputes agree everywhere
        assert fr(got, k) == repair(fr(got, k)) or k.startswith("udp_ffff"), k


@pytest.mark.gpu
def test_gpu_rewrite_identity(zp):
    """rewrite(extract(all writable)) leaves a c6 arena byte-identical."""
    import torch
    d = torch.device("cuda:0")
    a, o, l_ = zp.batch.generate("c6", 20000, first=123, device=d)
    before = a.clone()
    recs, _ = zp.batch.parse_batch(a, o, l_)
    cols = zp.columns.extract(a, o, l_, recs, names=list(zp.columns.WRITABLE))
    zp.columns.rewrite(a, o, l_, recs, cols)
    torch.cuda.synchronize()
    assert torch.equal(a, before)


@pytest.mark.gpu
def test_gpu_rewrite_far_l4(zp):
    """A far-L4 record (L4 past byte 262,143): the Ethernet header length is
    re-derived from the frame; port and address writes."""
    from test_l4_far import deep_frame
    from test_columns import pack
    frame, off = deep_frame(6601, l4="udp", vlan=True, outer_chain=True)
    assert off > 0x3FFFF
    near = edge_frames()[-1]
    arena, offs, lens = pack([near, frame, near])
    cols = random_cols(np.random.default_rng(2), 3,
                       ("src_port", "dest_port", "src_addr", "dest_addr", "vlan_tci"))
    _, changed, orec = run_rewrite(zp, arena, offs, lens, cols)
    assert orec["err"][1] == 0 and orec["l4_off"][1] == off
    assert all(c[1] for c in changed.values())


@pytest.mark.gpu
def test_gpu_rewrite_stream_and_facade_checks(zp):
    """columns.rewrite on a non-default stream; its argument checks."""
    import torch
    d = torch.device("cuda:0")
    arena, offs, lens = zp.batch.generate_host("c5", 1500, first=9)
    cols = random_cols(np.random.default_rng(8), 1500, NAT)
    run_rewrite(zp, arena, offs, lens, cols, stream=torch.cuda.Stream(d))
    a = torch.from_numpy(arena).to(d)
    o = torch.from_numpy(offs.astype(np.int64)).to(d)
    l_ = torch.from_numpy(lens.astype(np.int32)).to(d)
    recs, _ = zp.batch.parse_batch(a, o, l_)
    before = a.clone()
    ttl = torch.zeros(1500, dtype=torch.uint8, device=d)
    bad = [{"ethertype": torch.zeros(1500, dtype=torch.uint16, device=d)},   # not writable
           {"nonsense": ttl}, {"ttl": ttl[:-1]}, {"ttl": ttl.to(torch.int32)},
           {"ttl": ttl.cpu()}, {"src_addr": torch.zeros((1500, 32), dtype=torch.uint8,
                                                        device=d)[:, :16]}]
    for c in bad:
        with pytest.raises(ValueError):
            zp.columns.rewrite(a, o, l_, recs, c)
    o2 = o.clone()
    o2[1] = o2[0]                                       # frames 0 and 1 overlap
    with pytest.raises(ValueError):
        zp.columns.rewrite(a, o2, l_, recs, {"ttl": ttl})
    torch.cuda.synchronize()
    assert torch.equal(a, before)


# ---- GPU: layouts, reuse of records, capture, overlap checks ---------------

def to_device(arena, offs, lens):
    import torch
    d = torch.device("cuda:0")
    return (torch.from_numpy(arena).to(d), torch.from_numpy(offs.astype(np.int64)).to(d),
            torch.from_numpy(lens.astype(np.int32)).to(d))


def tcp6_bare():
    """Ethernet / IPv6 / TCP without payload: 74 B, the TCP header's last
    byte is the frame's last."""
    f = repair(_eth(0x86DD) + _ip6(6, _tcp(4000, 443, b"")))
    assert len(f) == 74 and orc.parse_one(f)[0] == 0
    return f


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["gapped", "reversed", "shuffled", "tight_end"])
def test_gpu_rewrite_layouts(zp, layout):
    """The ABI puts frames anywhere: 700 c5 frames with 1-23 bytes of non-zero
    filler between them (which must survive), the descriptors ascending,
    reversed or shuffled; and a back-to-back batch whose last frame, a 74-B
    TCP/IPv6 segment without payload, ends on the allocation's last byte."""
    ha, ho, hl = zp.batch.generate_host("c5", 700, first=31)
    frames = [ha[int(o):int(o) + int(l)].tobytes() for o, l in zip(ho, hl)]
    rng = np.random.default_rng(17)
    tight = layout == "tight_end"
    if tight:
        frames.append(tcp6_bare())
    gaps = np.zeros(len(frames), np.int64) if tight else rng.integers(1, 24, len(frames))
    lens = np.array([len(f) for f in frames], np.uint32)
    offs = (np.cumsum(gaps) + np.concatenate([[0], np.cumsum(lens[:-1], dtype=np.int64)])
            ).astype(np.uint64)
    end = int(offs[-1] + lens[-1])
    arena = rng.integers(1, 256, end + (0 if tight else 9), dtype=np.uint8)
    owned = np.zeros(len(arena), bool)
    for o, f in zip(offs, frames):
        arena[int(o):int(o) + len(f)] = np.frombuffer(f, np.uint8)
        owned[int(o):int(o) + len(f)] = True
    if layout == "reversed":
        offs, lens = offs[::-1].copy(), lens[::-1].copy()
    elif layout == "shuffled":
        p = rng.permutation(len(offs))
        offs, lens = offs[p], lens[p]
    assert (frames_at(offs, lens, offs.astype(np.int64) + 5) == np.arange(len(offs))).all()
    cols = random_cols(np.random.default_rng(23), len(offs), WRITABLE)
    got, changed, orec = run_rewrite(zp, arena, offs, lens, cols, guard=0 if tight else 64)
    assert (orec["err"] == 0).all() and all(changed[k].any() for k in WRITABLE)
    assert tight or ((~owned).sum() > 700 and np.array_equal(got[~owned], arena[~owned])
                     and got[~owned].all())
    if tight:
        assert int(offs[-1] + lens[-1]) == len(arena) and lens[-1] == 74
        assert all(changed[k][-1] for k in ("src_port", "tcp_window", "src_addr"))


@pytest.mark.gpu
def test_gpu_rewrite_reuses_records(zp):
    """Semantics 5, three times over: successive rewrites of one c6 batch with
    the records of the one parse (all 14 columns, the NAT set, the ports),
    each equal to rewrite_ref applied in turn; a GPU parse afterwards gives
    the original records, and a GPU extract the last-written values."""
    import torch
    arena, offs, lens = zp.batch.generate_host("c6", 2000, first=3)
    orec, oext = orc.parse_batch(arena, offs, lens)
    a, o, l_ = to_device(arena, offs, lens)
    recs, _ = zp.batch.parse_batch(a, o, l_)
    packed = orc.pack(orec, oext).tobytes()
    assert recs.cpu().numpy().tobytes() == packed
    want, last = arena, {}
    for k, names in enumerate([WRITABLE, NAT, ("src_port", "dest_port")]):
        cols = random_cols(np.random.default_rng(70 + k), len(offs), names)
        zp.columns.rewrite(a, o, l_, recs, {c: torch.from_numpy(v).to(a.device)
                                            for c, v in cols.items()})
        want, changed, applied = rewrite_batch_ref(want, offs, lens, orec, oext, cols)
        bad = np.nonzero(a.cpu().numpy() != want)[0]
        assert bad.size == 0, (k, bad[:8], frames_at(offs, lens, bad[:8]))
        assert all(changed[c].any() for c in names)
        for c in names:
            last[c] = (as_extracted(c, cols[c], orec), applied[c])
    recs2, _ = zp.batch.parse_batch(a, o, l_)
    got = zp.columns.extract(a, o, l_, recs2, names=list(WRITABLE))
    torch.cuda.synchronize()
    assert recs2.cpu().numpy().tobytes() == packed
    assert torch.equal(recs, recs2)                       # and the rewrite left its input alone
    for c, (wr, m) in last.items():
        assert m.any() and np.array_equal(got[c].cpu().numpy()[m], wr[m]), c


@pytest.mark.gpu
def test_gpu_rewrite_check_false_under_capture(zp):
    """columns.rewrite(check=False) neither reduces nor synchronises, so one
    torch.cuda.graph holds it (a single kernel); replayed twice with the
    column tensors edited in place in between, the arena is rewrite_ref
    applied twice."""
    import torch
    arena, offs, lens = zp.batch.generate_host("c5", 1500, first=44)
    orec, oext = orc.parse_batch(arena, offs, lens)
    a, o, l_ = to_device(arena, offs, lens)
    recs, _ = zp.batch.parse_batch(a, o, l_)
    first = random_cols(np.random.default_rng(91), 1500, NAT)
    second = random_cols(np.random.default_rng(92), 1500, NAT)
    tc = {c: torch.from_numpy(v).to(a.device) for c, v in first.items()}
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        zp.columns.rewrite(a, o, l_, recs, tc, check=False)
    torch.cuda.synchronize()
    assert np.array_equal(a.cpu().numpy(), arena)         # capturing ran nothing
    g.replay()
    torch.cuda.synchronize()
    want, _, _ = rewrite_batch_ref(arena, offs, lens, orec, oext, first)
    assert np.array_equal(a.cpu().numpy(), want)
    for c, v in second.items():
        tc[c].copy_(torch.from_numpy(v))
    g.replay()
    torch.cuda.synchronize()
    want2, changed, _ = rewrite_batch_ref(want, offs, lens, orec, oext, second)
    assert np.array_equal(a.cpu().numpy(), want2) and all(c.any() for c in changed.values())


@pytest.mark.gpu
def test_gpu_rewrite_disjoint_edges(zp):
    """columns.rewrite's overlap check: frames that touch are accepted; a
    one-byte overlap, a frame inside another and a duplicate descriptor raise
    ValueError before anything is written."""
    import torch
    arena, offs, lens = zp.batch.generate_host("c5", 300, first=12)
    assert (np.diff(offs.astype(np.int64)) == lens[:-1]).all()           # every pair touches
    cols = random_cols(np.random.default_rng(3), 300, NAT)
    run_rewrite(zp, arena, offs, lens, cols)
    a, o, l_ = to_device(arena, offs, lens)
    recs, _ = zp.batch.parse_batch(a, o, l_)
    tc = {c: torch.from_numpy(v).to(a.device) for c, v in cols.items()}
    before = a.clone()
    big = int(np.argmax(lens[:-1]))
    assert lens[big] >= 200
    one_byte, inside, dup = o.clone(), o.clone(), o.clone()
    one_byte[7] -= 1                                      # frame 7 starts on frame 6's last byte
    inside[big + 1] = o[big] + 10                         # a 64-B descriptor inside frame `big`
    l_in = l_.clone()
    l_in[big + 1] = 64
    dup[9] = o[8]
    l_dup = l_.clone()
    l_dup[9] = l_[8]
    for oo, ll in ((one_byte, l_), (inside, l_in), (dup, l_dup)):
        with pytest.raises(ValueError):
            zp.columns.rewrite(a, oo, ll, recs, tc)
    torch.cuda.synchronize()
    assert torch.equal(a, before)
