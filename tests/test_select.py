"""Select and gather (zp_select_device, zp_gather_frames_device, select.py).

CPU: tests/select_ref.py pinned on the golden packets by hand-written
expectations, the encoding of Select.where, and every refusal of the C ABI
(they return before any HIP call).
GPU: every result equals select_ref exactly; idx is compared as an array,
which also proves the compaction stable.
"""
import os
import random
import re

import numpy as np
import pytest

import oracle as orc
import select_ref as ref
from test_columns import frames_corpus, pack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPEC = {name: (dt, w) for name, dt, w in orc.COLUMN_SPEC}
NAMES = [c[0] for c in orc.COLUMN_SPEC]
BYTE_ARRAYS = [name for name, dt, w in orc.COLUMN_SPEC if w > 1]


def golden_batch(golden):
    frames = [bytes.fromhex(fx["bytes"]) for fx in golden["fixtures"]]
    arena, offs, lens = pack(frames)
    recs, ext = orc.parse_batch(arena, offs, lens)
    return arena, offs, lens, recs, ext, orc.columns(arena, offs, lens, recs), orc.pack(recs, ext)


# ---- CPU: the reference pinned by hand --------------------------------------

def test_reference_on_the_golden_packets(zp, golden):
    S = zp.select.Select
    arena, offs, lens, recs, ext, cols, packed = golden_batch(golden)
    name = [fx["name"] for fx in golden["fixtures"]]
    assert name[6] == "ipv6_routing_extension_header" and name[18] == "icmpv4_in_ipv4_in_ethernet"

    def sel(s):
        return list(np.flatnonzero(ref.select_mask(s.encode(), cols, packed, lens)))
    tcp = [6, 7, 8, 12, 23]                       # the fixtures with a TcpReader
    assert sel(S(has=("tcp",))) == tcp
    assert sel(S().where("l4_proto", eq=6)) == tcp
    assert sel(S().where("dest_port", eq=33441)) == [5]
    assert sel(S().where("dest_port", eq=5678)) == [1, 2]
    assert sel(S(has=("tcp",)).where("dest_port", eq=43424)) == [6, 12]
    assert sel(S().where("dest_port", eq=43424).where("src_port", eq=8080)
               .where("inner_version", eq=0)) == [6]
    assert sel(S().where("src_addr", prefix="192.168.0.0/24")) == [1, 2]
    assert sel(S().where("src_addr", prefix="192.168.1.0/24")) == [20, 21]
    assert sel(S().where("src_addr", prefix="192.168.0.0/16")) == [1, 2, 20, 21]
    assert sel(S().where("src_addr", prefix="10.0.0.0/8")) == [13, 14]
    assert sel(S().where("src_addr", prefix="fc00::/8")) == [6, 12]
    assert sel(S().where("inner_dest_addr", prefix="2001:db8::/32")) == [13]
    assert sel(S().where("vlan_tci", between=(150, 250))) == [2, 21, 22, 23]
    assert sel(S(ok=True).where("vlan_tci", outside=(150, 250))) == \
        [i for i in range(24) if i not in (0, 15, 16, 17, 18, 2, 21, 22, 23)]
    assert sel(S().where("icmp_type", eq=128)) == [9, 13, 22]
    assert sel(S().where("src_mac", mac="34:97:f6:94:02:0f")) == [19, 21, 22, 23]
    assert sel(S().where("ttl", eq=0x40, mask=0xC0)) == [1, 2, 7, 8, 11, 20, 21]
    # error fixtures: all columns read 0, so only err (and "equals 0" terms) select them
    bad = [0, 15, 16, 17, 18]
    assert sel(S(ok=False)) == bad
    assert sel(S(err=12)) == [18] and sel(S(err="IPV4_TOTAL_LENGTH")) == [18]
    assert sel(S(err=1)) == [0, 15, 16, 17]
    for col in NAMES:
        dt, w = SPEC[col]
        s = S().where(col, ne=bytes(w) if w > 1 else 0)
        assert not set(sel(s)) & set(bad), col
    assert sel(S(ok=True)) == [i for i in range(24) if i not in bad]
    assert sel(S(lacks=("ipv6", "ipv4"))) == bad           # an error record has no flags
    assert sel(S(ok=True, any_of=("icmpv4", "icmpv6"))) == [3, 4, 9, 13, 14, 22]
    assert sel(S(min_len=134, max_len=190)) == [6, 12, 13, 14]
    # compaction
    m = ref.select_mask(S(has=("tcp",)).encode(), cols, packed, lens)
    idx, po, c, total = ref.compact(m, lens)
    assert list(idx) == tcp and c == 5 and list(po) == [0, 150, 232, 314, 504] and total == 804
    assert ref.mask_words(m)[0] == sum(1 << i for i in tcp)
    assert ref.packed_bytes(arena, offs, lens, idx).tobytes() == b"".join(
        bytes.fromhex(golden["fixtures"][i]["bytes"]) for i in tcp)


def test_where_encoding_round_trips(zp):
    S, sl = zp.select.Select, zp.select
    cases = [("ttl", 1), ("dest_port", 2), ("tcp_seq", 4), ("src_mac", 6), ("src_addr", 16)]
    for name, w in cases:
        assert zp.columns.width(name) == w
        val = bytes(range(1, w + 1))
        msk = bytes([0xF0 | k for k in range(w)])
        iv, im = int.from_bytes(val, "little"), int.from_bytes(msk, "little")
        ops = [(dict(eq=val if w > 4 else iv), sl.MASK_EQ, val, b"\xff" * w),
               (dict(ne=val if w > 4 else iv), sl.MASK_NE, val, b"\xff" * w),
               (dict(eq=val if w > 4 else iv, mask=msk if w > 4 else im), sl.MASK_EQ, val, msk)]
        if w <= 4:
            ops += [(dict(between=(3, iv)), sl.RANGE, (3).to_bytes(w, "little"), val),
                    (dict(outside=(3, iv)), sl.NOT_RANGE, (3).to_bytes(w, "little"), val)]
        for kw, op, a, b in ops:
            e = S().where(name, **kw).encode()[0]
            t = e["terms"][0]
            assert e["nterms"] == 1 and t["col"] == zp.columns.INDEX[name] and t["op"] == op
            assert bytes(t["a"]) == a + bytes(16 - w) and bytes(t["b"]) == b + bytes(16 - w)
            assert not t["pad"].any()
    t = S().where("src_addr", prefix="10.0.0.0/8").encode()[0]["terms"][0]
    assert bytes(t["a"]) == bytes([10]) + bytes(15) and bytes(t["b"]) == bytes([255]) + bytes(15)
    t = S().where("dest_addr", prefix="2001:db8::/32").encode()[0]["terms"][0]
    assert bytes(t["a"]) == bytes.fromhex("20010db8") + bytes(12)
    assert bytes(t["b"]) == b"\xff" * 4 + bytes(12)
    t = S().where("dest_mac", mac="aa:bb:cc:dd:ee:ff").encode()[0]["terms"][0]
    assert bytes(t["a"][:6]) == bytes.fromhex("aabbccddeeff") and bytes(t["b"][:6]) == b"\xff" * 6
    e = S(ok=True, has=("tcp", "ipv4"), lacks=("ip_in_ip",), any_of=("ext",), min_len=60,
          max_len=1500).encode()[0]
    R = zp.records
    assert (e["flags_all"], e["flags_none"], e["flags_any"]) == \
        (R.F_TCP | R.F_IPV4, R.F_IP_IN_IP, R.F_EXT)
    assert (e["err"], e["min_len"], e["max_len"], e["nterms"]) == (0, 60, 1500, 0)
    assert S().encode()[0]["err"] == sl.ERR_ANY and S(ok=False).encode()[0]["err"] == sl.ERR_NONZERO
    assert S().encode()[0]["max_len"] == 0xFFFFFFFF
    for bad in (lambda: S().where("nope", eq=1), lambda: S().where("ttl", eq=256),
                lambda: S().where("src_mac", between=(1, 2)), lambda: S().where("ttl"),
                lambda: S().where("ttl", eq=1, ne=2), lambda: S().where("ttl", prefix="10.0.0.0/8"),
                lambda: S().where("src_addr", eq=5), lambda: S().where("src_addr", eq=bytes(4)),
                lambda: S(has=("tcpp",)), lambda: S(ok=True, err=3), lambda: S(err="NOPE")):
        with pytest.raises(ValueError):
            bad()
    s = S()
    for _ in range(sl.MAX_TERMS):
        s.where("ttl", eq=1)
    with pytest.raises(ValueError):
        s.where("ttl", eq=1)
    # the implementation's constants as the header states them
    hdr = open(os.path.join(ROOT, "include", "zero_packet.h")).read()
    assert int(re.search(r"#define ZP_SELECT_SCAN_FRAMES (\d+)u", hdr).group(1)) == sl.SCAN_FRAMES
    assert int(re.search(r"#define ZP_SELECT_MAX_TERMS (\d+)", hdr).group(1)) == sl.MAX_TERMS


def test_refusals_touch_no_device(zp):
    """Every refusal returns negative with its cause named, before any HIP
    call: the pointers given are never dereferenced."""
    lib, sl = zp._lib.hip(), zp.select
    P = 4096                                             # a non-null "device pointer"
    big = int(lib.zp_select_scratch_bytes(1000))
    assert lib.zp_select_scratch_bytes(0) < big < lib.zp_select_scratch_bytes(1 << 20)
    # one more scan span from ZP_SELECT_SCAN_FRAMES + 1 frames on
    step = lambda n: int(lib.zp_select_scratch_bytes(n + 1)) - int(lib.zp_select_scratch_bytes(n))
    assert step(sl.SCAN_FRAMES) == 8 * (1 + 2 + 2) and step(sl.SCAN_FRAMES - 1) == 0

    def call(enc, arena=P, offs=P, lens=P, recs=P, n=1000, mask=None, idx=P, packed=None,
             count=P, scratch=P, nscratch=big):
        return lib.zp_select_device(arena, offs, lens, recs, n,
                                    enc.ctypes.data if enc is not None else None, mask, idx,
                                    packed, count, scratch, nscratch, None)

    def refused(what, *a, **kw):
        assert call(*a, **kw) < 0, what
        assert what in lib.zp_last_error().decode(), (what, lib.zp_last_error())
    ok = sl.Select(ok=True).where("ttl", eq=3).encode()
    refused("null selector", None)
    refused("null count", ok, count=None)
    refused("null records", ok, recs=None)
    refused("scratch", ok, scratch=None)
    refused("scratch", ok, nscratch=big - 1)
    refused("terms need arena", ok, arena=None)
    refused("terms need arena", ok, lens=None)
    e = ok.copy(); e["nterms"] = 9
    refused("ZP_SELECT_MAX_TERMS", e)
    e = ok.copy(); e["terms"][0][0]["col"] = len(NAMES)
    refused("out of range", e)
    e = ok.copy(); e["terms"][0][0]["pad"][4] = 1
    refused("pad", e)
    e = ok.copy(); e["terms"][0][0]["op"] = 4
    refused("unknown op", e)
    for name in BYTE_ARRAYS:
        for op in (sl.RANGE, sl.NOT_RANGE):
            e = ok.copy(); e["terms"][0][0]["col"] = NAMES.index(name); e["terms"][0][0]["op"] = op
            refused("RANGE on byte-array", e)
    plain = sl.Select(ok=True).encode()
    refused("2^32", plain, n=1 << 32, nscratch=1 << 62)
    refused("need lens", plain, lens=None, packed=P)
    refused("need lens", sl.Select(min_len=1).encode(), lens=None)
    # gather
    g = lambda **kw: lib.zp_gather_frames_device(*[kw.get(k, P) for k in (
        "arena", "offs", "lens", "recs", "ext", "n", "idx", "packed", "m", "count", "dst",
        "dst_bytes", "out_offs", "out_lens", "out_recs", "out_ext", "stream")])
    base = dict(n=10, m=10, ext=None, out_ext=None, stream=None, count=None)
    assert g(**base, idx=None) < 0 and "null idx" in lib.zp_last_error().decode()
    assert g(**base, packed=None) < 0 and "packed_offs" in lib.zp_last_error().decode()
    assert g(**{**base, "out_ext": P}) < 0 and "out_ext needs ext" in lib.zp_last_error().decode()
    assert g(**{**base, "m": 0}) == 0                     # nothing to do, nothing launched


# ---- GPU --------------------------------------------------------------------

SENT_I, SENT_P = -7, -9


def dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def to_dev(*arrays):
    import torch
    out = []
    for a in arrays:
        a = np.ascontiguousarray(a)
        if a.dtype == np.uint64:
            a = a.astype(np.int64)
        elif a.dtype == np.uint32:
            a = a.astype(np.int32)
        elif a.dtype.fields is not None:
            a = a.view(np.uint8).reshape(len(a), -1)
        out.append(torch.from_numpy(a).to(dev()))
    return out


class Batch:
    """A host batch with the oracle's view of it and its device copy."""

    def __init__(self, arena, offs, lens):
        self.arena, self.offs, self.lens = arena, np.asarray(offs, np.uint64), \
            np.asarray(lens, np.uint32)
        self.n = len(self.offs)
        self.recs, self.ext = orc.parse_batch(arena, self.offs, self.lens)
        self.cols = orc.columns(arena, self.offs, self.lens, self.recs)
        self.packed = orc.pack(self.recs, self.ext)
        self.d = None

    def device(self):
        if self.d is None:
            self.d = to_dev(self.arena, self.offs, self.lens, self.packed)
        return self.d


def check_select(zp, b, sel, want=("idx", "packed_offs", "mask"), use_arena=True, use_lens=True):
    """Runs sel on the device and compares everything with select_ref."""
    import torch
    da, do, dl, dr = b.device()
    n = b.n
    out = {"idx": torch.full((n,), SENT_I, dtype=torch.int32, device=dev()),
           "packed_offs": torch.full((n,), SENT_P, dtype=torch.int64, device=dev()),
           "count": torch.full((2,), -1, dtype=torch.int64, device=dev())}
    s = zp.select.run(da if use_arena else None, do if use_arena else None,
                      dl if use_lens else None, dr, sel, want=want, out=out)
    enc = sel.encode()
    m = ref.select_mask(enc, b.cols, b.packed, b.lens if use_lens else None)
    idx, po, c, total = ref.compact(m, b.lens if use_lens else None)
    assert s.count.tolist() == [c, total], (s.count.tolist(), c, total)
    if "idx" in want:
        got = s.idx.cpu().numpy()
        assert np.array_equal(got[:c].astype(np.uint32), idx)
        assert (got[c:] == SENT_I).all(), "idx written past count"
    if "packed_offs" in want:
        got = s.packed_offs.cpu().numpy()
        assert np.array_equal(got[:c].astype(np.uint64), po)
        assert (got[c:] == SENT_P).all(), "packed_offs written past count"
    if "mask" in want:
        assert np.array_equal(s.mask.cpu().numpy().view(np.uint64), ref.mask_words(m))
    return s, m


def synthetic(n, seed):
    """n records whose flag bits are set by hand, with random lens: the
    record-only selectors pick any subset without reading a frame."""
    rng = np.random.default_rng(seed)
    R = Batch.__new__(Batch)
    R.n, R.arena, R.offs = n, np.zeros(16, np.uint8), np.zeros(n, np.uint64)
    R.lens = rng.integers(0, 70000, n).astype(np.uint32)
    R.lens[rng.integers(0, n)] = 0xFFFFFFF0              # sums pass 2^32
    i = np.arange(n)
    flags = np.full(n, 1, np.uint32)                     # ethernet
    flags |= np.where(i == 0, 1 << 6, 0).astype(np.uint32)          # tcp: only frame 0
    flags |= np.where(i == n - 1, 1 << 7, 0).astype(np.uint32)      # udp: only frame n - 1
    flags |= np.where(i % 2 == 1, 1 << 8, 0).astype(np.uint32)      # icmpv4: every other
    flags |= np.where(rng.random(n) < 0.5, 1 << 9, 0).astype(np.uint32)   # icmpv6: a random half
    R.packed = np.zeros(n, orc.PACKED_DTYPE)
    R.packed["flags"] = flags
    R.cols, R.d = None, None
    return R


SIZES = [1, 63, 64, 65, 255, 256, 257]


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES + ["span+1"])
def test_sizes_record_only(zp, n):
    S = zp.select.Select
    if n == "span+1":
        n = zp.select.SCAN_FRAMES + 1                    # one frame past a scan workgroup's span
        lib = zp._lib.hip()
        assert lib.zp_select_scratch_bytes(n) - lib.zp_select_scratch_bytes(n - 1) == 40
    b = synthetic(n, n)
    for name, sel in (("none", S(has=("arp",))), ("all", S(has=("ethernet",))),
                      ("first", S(has=("tcp",))), ("last", S(has=("udp",))),
                      ("every other", S(has=("icmpv4",))), ("random half", S(has=("icmpv6",)))):
        _, m = check_select(zp, b, sel, use_arena=False)
        if name in ("first", "last"):
            assert list(np.flatnonzero(m)) == [0 if name == "first" else n - 1]
        assert m.sum() == {"none": 0, "all": n}.get(name, m.sum())
    check_select(zp, b, S(has=("icmpv6",)), want=("idx",), use_arena=False, use_lens=False)
    check_select(zp, b, S(has=("icmpv6",)), want=("mask",), use_arena=False)
    check_select(zp, b, S(has=("icmpv6",)), want=(), use_arena=False)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES + ["span+1"])
def test_sizes_with_terms(zp, n):
    """The same sizes through the term kernel, on generated frames (c3; the
    64-B frames of c2 for the size past a scan workgroup's span). No selector
    picks "every other frame" from real frames: bit 0 of the L4 checksum
    stands in for it and for the random half."""
    S = zp.select.Select
    cfg = "c3"
    if n == "span+1":
        n, cfg = zp.select.SCAN_FRAMES + 1, "c2"
    b = Batch(*zp.batch.generate_host(cfg, n, first=5))
    assert (b.recs["err"] == 0).all() and (b.cols["l4_proto"] != 0).all()

    def only(i):
        c = b.cols
        return (S().where("l4_checksum", eq=int(c["l4_checksum"][i]))
                .where("ip_id", eq=int(c["ip_id"][i])).where("src_port", eq=int(c["src_port"][i]))
                .where("src_addr", eq=bytes(c["src_addr"][i])))
    for name, sel in (("none", S().where("ip_version", eq=0)),
                      ("all", S().where("ttl", between=(0, 255))),
                      ("first", only(0)), ("last", only(n - 1)),
                      ("half", S().where("l4_checksum", eq=1, mask=1))):
        _, m = check_select(zp, b, sel)
        if name in ("first", "last"):
            assert list(np.flatnonzero(m)) == [0 if name == "first" else n - 1]
        elif name == "half" and n > 64:
            both_sides(m)
        else:
            assert m.sum() == {"none": 0, "all": n}.get(name, m.sum())


_corpus = {}


def corpus(zp, golden, key="mixed"):
    """Golden frames, generated c3-c6 frames and their mutations (two thirds
    checksum-refilled), gapped: every reader and many error codes occur."""
    if key not in _corpus:
        if key == "mixed":
            frames = frames_corpus(zp, golden, 1800, seed=7)
        else:                                            # one generated config, mutated
            from fuzzfix import repair
            from test_oracle_fuzz import mutate
            rng = random.Random(31)
            arena, offs, lens = zp.batch.generate_host(key, 500, first=777)
            seeds = [arena[o:o + l].tobytes() for o, l in zip(offs, lens)]
            frames = list(seeds)
            for _ in range(700):
                f = mutate(rng, rng.choice(seeds))
                frames.append(repair(f) if rng.random() < 2 / 3 else f)
        _corpus[key] = Batch(*pack(frames))
    return _corpus[key]


def test_corpus_has_both_sides(zp, golden):
    """CPU: every column of the mixed corpus has at least two values, and of
    c4, c5 and c6 each has the readers the term tests below rely on."""
    b = corpus(zp, golden)
    for name in NAMES:
        v = b.cols[name].reshape(b.n, -1)
        assert len(np.unique(v, axis=0)) >= 2, name
    assert len(np.unique(b.recs["err"])) >= 8
    for cfg in ("c4", "c5", "c6"):
        c = corpus(zp, golden, cfg)
        assert (c.recs["err"] == 0).sum() > 300 and (c.recs["err"] != 0).sum() > 50


def threshold(col):
    """The median of the column's distinct values (>= 2 of them): both
    `== t` / `>= t` and their complements are non-empty."""
    d = np.unique(col.reshape(len(col), -1), axis=0)
    assert len(d) >= 2
    return d[len(d) // 2], d[-1]


def both_sides(m):
    assert m.any() and not m.all(), "the reference must select some frames and leave some out"


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_one_term_of_every_op(zp, golden, name):
    b = corpus(zp, golden)
    S = zp.select.Select
    dt, w = SPEC[name]
    t, top = threshold(b.cols[name])
    if w > 1:
        val = bytes(t)
        m = bytes([0xFF] * (w - 1) + [0xF0])
        sels = [S().where(name, eq=val), S().where(name, ne=val),
                S().where(name, eq=bytes(x & y for x, y in zip(val, m)), mask=m)]
    else:
        t, top = int(t[0]), int(top[0])
        sels = [S().where(name, eq=t), S().where(name, ne=t),
                S().where(name, between=(t, top)), S().where(name, outside=(t, top)),
                S().where(name, eq=t & 0x0F, mask=0x0F)]
    for k, sel in enumerate(sels):
        _, m = check_select(zp, b, sel)
        if k < 4 and not (w > 1 and k == 2):
            both_sides(m)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", ["c4", "c5", "c6"])
def test_terms_on_generated_configs(zp, golden, cfg):
    """Mutated, checksum-refilled c4 / c5 / c6 frames: 5-tuple terms, an 8-term
    conjunction, and terms combined with the record predicate."""
    b = corpus(zp, golden, cfg)
    S = zp.select.Select
    okm = b.recs["err"] == 0
    port, _ = threshold(b.cols["dest_port"][okm & (b.cols["dest_port"] != 0)])
    ttl, ttl_top = threshold(b.cols["ttl"][okm])
    both_sides(check_select(zp, b, S(ok=True).where("dest_port", between=(int(port[0]), 65535)))[1])
    both_sides(check_select(zp, b, S().where("l4_proto", eq=17)
                            .where("src_port", between=(1, 40000)))[1])
    i = int(np.flatnonzero(okm & (b.cols["l4_proto"] != 0))[5])
    c = b.cols
    eight = (S(ok=True).where("src_addr", eq=bytes(c["src_addr"][i]))
             .where("dest_addr", eq=bytes(c["dest_addr"][i]))
             .where("src_port", eq=int(c["src_port"][i])).where("dest_port", eq=int(c["dest_port"][i]))
             .where("l4_proto", eq=int(c["l4_proto"][i])).where("ip_version", eq=int(c["ip_version"][i]))
             .where("ttl", between=(0, 255)).where("src_mac", mac=bytes(c["src_mac"][i])))
    _, m = check_select(zp, b, eight)
    assert m[i] and not m.all()
    both_sides(check_select(zp, b, S(has=("ipv6",), min_len=80).where("ttl", between=(int(ttl[0]), 255)))[1])
    both_sides(check_select(zp, b, S(ok=False).where("ttl", eq=0))[1])


@pytest.mark.gpu
def test_prefix_aliasing_and_the_ip_version_fix(zp, golden):
    """A /8 over IPv4 also matches an IPv6 address that starts with the same
    byte: the documented aliasing; an ip_version term tells them apart."""
    from pybuilder import internet_checksum, pseudo_header
    b0 = corpus(zp, golden, "c5")
    frames = [b0.arena[int(o):int(o) + int(l)].tobytes() for o, l in zip(b0.offs, b0.lens)]
    # an accepted IPv6 + UDP frame of the golden set, its source rewritten to 0a..:
    f = bytearray(bytes.fromhex(golden["fixtures"][5]["bytes"]))
    assert golden["fixtures"][5]["name"] == "ipv6_udp_payload"
    f[22] = 0x0A
    f[60:62] = b"\0\0"
    ck = internet_checksum(bytes(f[54:]), pseudo_header(bytes(f[22:38]), bytes(f[38:54]), 17, len(f) - 54))
    f[60:62] = ck.to_bytes(2, "big")
    # and the IPv4 frames of the batch moved into 10/8 would need new checksums: use the
    # golden ipv4_in_ipv4 frame (10.0.0.1 -> 10.0.0.2) instead
    v4 = bytes.fromhex(golden["fixtures"][14]["bytes"])
    b = Batch(*pack(frames[:300] + [bytes(f), v4] + frames[300:600]))
    assert b.recs["err"][300] == 0 and b.recs["err"][301] == 0
    S = zp.select.Select
    _, m = check_select(zp, b, S().where("src_addr", prefix="10.0.0.0/8"))
    assert m[300] and m[301], "the /8 matches the IPv6 address too (aliasing)"
    _, m = check_select(zp, b, S().where("src_addr", prefix="10.0.0.0/8").where("ip_version", eq=4))
    assert m[301] and not m[300]
    _, m = check_select(zp, b, S().where("src_addr", prefix="a00::/8").where("ip_version", eq=6))
    assert m[300] and not m[301]
    # an IPv6 /32 on the same batch: the rewritten frame's own
    a6 = bytes(b.cols["src_addr"][300])
    p = ":".join(f"{a6[k] << 8 | a6[k + 1]:x}" for k in (0, 2)) + "::/32"
    _, m = check_select(zp, b, S().where("src_addr", prefix=p))
    assert m[300] and not m[301] and not m.all()


@pytest.mark.gpu
def test_record_only_on_fuzzed_batches(zp, golden):
    S = zp.select.Select
    for cfg in ("c5", "c6"):
        b = corpus(zp, golden, cfg)
        errs = np.unique(b.recs["err"])
        assert len(errs) >= 4
        sels = [S(has=("tcp",)), S(has=("ipv4", "udp")), S(lacks=("ipv6",)), S(ok=True, lacks=("tcp", "udp")),
                S(any_of=("icmpv4", "icmpv6", "arp")), S(ok=True), S(ok=False), S(),
                S(min_len=100), S(max_len=99), S(ok=True, min_len=64, max_len=200),
                S(ok=True, has=("ethernet",), any_of=("tcp", "udp"), lacks=("ip_in_ip",), min_len=70)]
        sels += [S(err=int(e)) for e in errs]
        for sel in sels:
            check_select(zp, b, sel, use_arena=False)                 # the arena passed as NULL
        check_select(zp, b, S(has=("udp",)), want=("idx",), use_arena=False, use_lens=False)
        da, do, dl, dr = b.device()
        counts = zp.stats.to_dict(zp.stats.count(dr))      # zp_stats_device's flag counts
        for x in ("ethernet", "tcp", "udp", "ipv6", "ip_in_ip", "ext"):
            s = zp.select.run(None, None, None, dr, S(has=(x,)), want=())
            assert int(s.count[0]) == counts[x], x


@pytest.mark.gpu
def test_far_l4_and_past_the_window(zp, golden):
    """The far-L4 frames of tests/test_l4_far.py and a c4 frame whose L4 header
    lies past the 112-B staged window."""
    from test_l4_far import _cases
    far = [f for f, _ in _cases()]
    c4 = corpus(zp, golden, "c4")
    deep = np.flatnonzero((c4.recs["err"] == 0) & (c4.recs["l4_off"] > 112))
    assert len(deep), "c4 has frames whose L4 header lies past the window"
    frames = far + [c4.arena[int(c4.offs[i]):int(c4.offs[i]) + int(c4.lens[i])].tobytes()
                    for i in list(deep[:20]) + list(range(40))]
    b = Batch(*pack(frames))
    assert (b.recs["err"][:len(far)] == 0).all() and (b.recs["l4_off"][:len(far)] > 0x3FFFF).any()
    S = zp.select.Select
    for name in ("l4_proto", "src_port", "dest_port", "icmp_type", "l4_checksum", "payload_off",
                 "inner_version", "inner_src_addr", "inner_protocol", "protocol", "ethertype",
                 "vlan_tci", "tcp_seq", "tcp_flags"):
        dt, w = SPEC[name]
        col = b.cols[name]
        for i in list(range(len(far))) + [len(far), len(far) + 1]:
            v = bytes(col[i]) if w > 1 else int(col[i])
            _, m = check_select(zp, b, S().where(name, eq=v))
            assert m[i]


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["gaps", "reverse", "shuffled", "dup"])
def test_layouts(zp, golden, layout):
    from test_gpu_parity import layout_batch
    b0 = corpus(zp, golden)
    frames = [b0.arena[int(o):int(o) + int(l)].tobytes() for o, l in zip(b0.offs, b0.lens)][:900]
    b = Batch(*layout_batch(frames, layout))
    S = zp.select.Select
    port, _ = threshold(b.cols["dest_port"])
    for sel in (S(ok=True).where("dest_port", between=(int(port[0]), 65535)),
                S().where("ip_version", eq=6).where("ttl", outside=(0, 32)),
                S(has=("udp",), min_len=80)):
        _, m = check_select(zp, b, sel)
        both_sides(m)
        s = zp.select.run(*b.device(), sel, want=("idx", "packed_offs"))
        a2, o2, l2, r2 = zp.select.gather(*b.device(), s)
        idx = np.flatnonzero(m)
        assert a2.cpu().numpy().tobytes() == ref.packed_bytes(b.arena, b.offs, b.lens, idx).tobytes()


# ---- GPU: gather ------------------------------------------------------------

@pytest.mark.gpu
def test_gather_view_and_packed(zp, golden):
    import torch
    b = corpus(zp, golden)
    da, do, dl, _ = b.device()
    dr, de = zp.batch.parse_batch(da, do, dl)
    assert dr.cpu().numpy().tobytes() == b.packed.tobytes()
    S = zp.select.Select
    for sel in (S(ok=True, any_of=("ext", "inner_ext")), S(ok=True).where("l4_proto", eq=6), S()):
        s, m = check_select(zp, b, sel, want=("idx", "packed_offs"))
        s = zp.select.run(da, do, dl, dr, sel, want=("idx", "packed_offs"))
        idx = np.flatnonzero(m)
        c = len(idx)
        assert c > 10
        # a view: the same arena, gathered descriptors
        a1, o1, l1, r1, e1 = zp.select.gather(da, do, dl, dr, s, ext=de, pack=False)
        assert a1 is da and o1.numel() == c
        assert np.array_equal(o1.cpu().numpy().astype(np.uint64), b.offs[idx])
        assert np.array_equal(l1.cpu().numpy().astype(np.uint32), b.lens[idx])
        assert r1.cpu().numpy().tobytes() == b.packed[idx].tobytes()
        assert torch.equal(e1, de[:, torch.from_numpy(idx).to(dev())])   # copied flagged or not
        # packed
        a2, o2, l2, r2, e2 = zp.select.gather(da, do, dl, dr, s, ext=de)
        want = ref.packed_bytes(b.arena, b.offs, b.lens, idx)
        assert a2.numel() == len(want) and a2.cpu().numpy().tobytes() == want.tobytes()
        assert np.array_equal(o2.cpu().numpy().astype(np.uint64), ref.compact(m, b.lens)[1])
        assert torch.equal(l2, l1) and torch.equal(r2, r1) and torch.equal(e2, e1)
        # the gathered batch parses to the gathered records; flagged ext entries equal
        r3, e3 = zp.batch.parse_batch(a2, o2, l2)
        assert torch.equal(r3, r2)
        got, gext = zp.batch.records_to_numpy(r2, e2)
        _, pext = zp.batch.records_to_numpy(r3, e3)
        assert zp.records.ext_match(gext, b.ext[:, idx], b.recs[idx])
        assert zp.records.ext_match(pext, b.ext[:, idx], b.recs[idx])
        cols = zp.columns.extract(a2, o2, l2, r2, names=["dest_port", "src_addr"])
        assert np.array_equal(cols["dest_port"].cpu().numpy(), b.cols["dest_port"][idx])
        assert np.array_equal(cols["src_addr"].cpu().numpy(), b.cols["src_addr"][idx])


def raw_gather(zp, da, do, dl, idx_t, po_t, m, count_t, dst_t, dst_off, dst_bytes, out_offs, out_lens):
    lib = zp._lib.hip()
    rc = lib.zp_gather_frames_device(
        da.data_ptr(), do.data_ptr(), dl.data_ptr(), None, None, do.numel(), idx_t.data_ptr(),
        po_t.data_ptr() if po_t is not None else None, m,
        count_t.data_ptr() if count_t is not None else None,
        dst_t.data_ptr() + dst_off if dst_t is not None else None, dst_bytes,
        out_offs.data_ptr(), out_lens.data_ptr(), None, None, None)
    zp._lib.check(rc, "zp_gather_frames_device")


@pytest.mark.gpu
def test_gather_edges_alignments_and_guards(zp):
    """Frames of 1, 15, 16, 17, 64 and 9,000 B (and an empty one), every source
    alignment against every destination alignment, guard bytes around dst."""
    import torch
    rng = np.random.default_rng(5)
    sizes = [1, 15, 16, 17, 64, 9000, 0, 1, 1, 3, 64, 64, 64, 33, 5, 2, 128, 47]
    for sa in range(16):
        frames = [rng.integers(1, 255, s, dtype=np.uint8).tobytes() for s in sizes]
        offs, pos = [], sa
        for k, f in enumerate(frames):
            offs.append(pos)
            pos += len(f) + (k * 7) % 16                 # every relative alignment occurs
        arena = np.zeros(pos + 64, np.uint8)
        for o, f in zip(offs, frames):
            arena[o:o + len(f)] = np.frombuffer(f, np.uint8)
        lens = np.array(sizes, np.uint32)
        da, do, dl = to_dev(arena, np.array(offs, np.uint64), lens)
        sel = np.array([k for k in range(len(sizes)) if k != 9], np.uint32)
        po = np.concatenate([[0], np.cumsum(lens[sel])[:-1]]).astype(np.uint64)
        total = int(lens[sel].sum())
        di, dp = to_dev(sel, po)
        want = ref.packed_bytes(arena, offs, lens, sel)
        for da_ in range(16):
            dst = torch.full((64 + 16 + total + 64,), 0xA5, dtype=torch.uint8, device=dev())
            oo = torch.zeros(len(sel), dtype=torch.int64, device=dev())
            ol = torch.zeros(len(sel), dtype=torch.int32, device=dev())
            start = 64 + (-(dst.data_ptr() + 64) % 16) + da_
            raw_gather(zp, da, do, dl, di, dp, len(sel), None, dst, start, total, oo, ol)
            h = dst.cpu().numpy()
            assert h[start:start + total].tobytes() == want.tobytes(), (sa, da_)
            assert (h[:start] == 0xA5).all() and (h[start + total:] == 0xA5).all(), (sa, da_)
            assert np.array_equal(oo.cpu().numpy().astype(np.uint64), po)
            assert np.array_equal(ol.cpu().numpy().astype(np.uint32), lens[sel])


@pytest.mark.gpu
@pytest.mark.parametrize("top", [70, 250, 300])
def test_gather_short_frames_many_workgroups(zp, top):
    """700 frames of 0..top bytes, every third left out: an average length on
    either side of the size at which the gather takes 256 entries per workgroup
    instead of 64, more than one workgroup either way."""
    import torch
    rng = np.random.default_rng(top)
    lens = rng.integers(0, top + 1, 700).astype(np.uint32)
    offs = (np.concatenate([[0], np.cumsum(lens + rng.integers(0, 9, 700))[:-1]]) + 5).astype(np.uint64)
    arena = rng.integers(1, 255, int(offs[-1] + lens[-1]) + 64, dtype=np.uint8)
    sel = np.array([k for k in range(700) if k % 3 != 1], np.uint32)
    po = np.concatenate([[0], np.cumsum(lens[sel])[:-1]]).astype(np.uint64)
    total = int(lens[sel].sum())
    da, do, dl, di, dp = to_dev(arena, offs, lens, sel, po)
    want = ref.packed_bytes(arena, offs, lens, sel)
    for shift in (0, 3):
        dst = torch.full((64 + 16 + total + 64,), 0xA5, dtype=torch.uint8, device=dev())
        oo = torch.zeros(len(sel), dtype=torch.int64, device=dev())
        ol = torch.zeros(len(sel), dtype=torch.int32, device=dev())
        start = 64 + (-(dst.data_ptr() + 64) % 16) + shift
        raw_gather(zp, da, do, dl, di, dp, len(sel), None, dst, start, total, oo, ol)
        h = dst.cpu().numpy()
        assert h[start:start + total].tobytes() == want.tobytes()
        assert (h[:start] == 0xA5).all() and (h[start + total:] == 0xA5).all()
        assert np.array_equal(ol.cpu().numpy().astype(np.uint32), lens[sel])


@pytest.mark.gpu
def test_gather_bounds_m_and_count(zp, golden):
    """m below, at and above *count, count == NULL, and a dst too small for
    the last frames: nothing is written past the entries handled or past dst."""
    import torch
    b = corpus(zp, golden, "c5")
    da, do, dl, dr = b.device()
    s = zp.select.run(da, do, dl, dr, zp.select.Select(ok=True), want=("idx", "packed_offs"))
    c, total = s.count.tolist()
    idx = s.idx.cpu().numpy()[:c]
    want = ref.packed_bytes(b.arena, b.offs, b.lens, idx)
    ends = np.cumsum(b.lens[idx].astype(np.int64))
    for m, count in ((c - 3, s.count), (c, s.count), (c + 50, s.count), (c - 3, None), (c, None)):
        k = min(m, c)
        dst = torch.full((64 + total + 64,), 0xA5, dtype=torch.uint8, device=dev())
        oo = torch.full((c + 50,), SENT_P, dtype=torch.int64, device=dev())
        ol = torch.full((c + 50,), SENT_I, dtype=torch.int32, device=dev())
        raw_gather(zp, da, do, dl, s.idx, s.packed_offs, m, count, dst, 64, total, oo, ol)
        h = dst.cpu().numpy()
        assert h[64:64 + ends[k - 1]].tobytes() == want[:ends[k - 1]].tobytes()
        assert (h[:64] == 0xA5).all() and (h[64 + ends[k - 1]:] == 0xA5).all()
        assert (oo.cpu().numpy()[k:] == SENT_P).all() and (ol.cpu().numpy()[k:] == SENT_I).all()
        assert np.array_equal(ol.cpu().numpy()[:k].astype(np.uint32), b.lens[idx[:k]])
    # a dst that ends inside frame c - 2: that frame and the last are not copied
    short = int(ends[c - 3]) + 5
    dst = torch.full((64 + total + 64,), 0xA5, dtype=torch.uint8, device=dev())
    oo = torch.zeros(c, dtype=torch.int64, device=dev())
    ol = torch.zeros(c, dtype=torch.int32, device=dev())
    raw_gather(zp, da, do, dl, s.idx, s.packed_offs, c, None, dst, 64, short, oo, ol)
    h = dst.cpu().numpy()
    assert h[64:64 + ends[c - 3]].tobytes() == want[:ends[c - 3]].tobytes()
    assert (h[64 + ends[c - 3]:] == 0xA5).all()


@pytest.mark.gpu
def test_rewrite_through_a_view(zp, golden):
    """columns.rewrite on a view sub-batch changes exactly the selected frames
    in the original arena."""
    import torch
    b = corpus(zp, golden, "c5")
    da, do, dl, dr = (t.clone() for t in b.device())
    sel = zp.select.Select(ok=True, has=("tcp",)).where("ip_version", eq=4)
    s, m = check_select(zp, b, sel, want=("idx",))
    s = zp.select.run(da, do, dl, dr, sel)
    a1, o1, l1, r1 = zp.select.gather(da, do, dl, dr, s, pack=False)
    ttl = zp.columns.extract(a1, o1, l1, r1, names=["ttl"])["ttl"]
    new = (ttl.to(torch.int32) - 1).clamp(min=1).to(torch.uint8)
    zp.columns.rewrite(a1, o1, l1, r1, {"ttl": new})
    after = da.cpu().numpy()
    r2, _ = zp.batch.parse_batch(da, do, dl)
    assert torch.equal(r2, dr), "records changed after the rewrite"
    got = zp.columns.extract(da, do, dl, r2, names=["ttl"])["ttl"].cpu().numpy()
    idx = np.flatnonzero(m)
    assert len(idx) > 20
    want = b.cols["ttl"].copy()
    want[idx] = np.maximum(want[idx].astype(np.int32) - 1, 1).astype(np.uint8)
    assert np.array_equal(got, want)
    changed = np.flatnonzero(after[:len(b.arena)] != b.arena)
    from test_rewrite import frames_at
    owners = set(frames_at(b.offs, b.lens, changed).tolist())
    assert owners and owners <= set(idx.tolist())


@pytest.mark.gpu
def test_enqueue_only_in_one_graph(zp, golden):
    """run(check=False) + gather(capacity=n) captured in one graph, replayed
    twice with another batch parsed into the same buffers in between: the
    results follow the data."""
    import torch
    b1, b2 = corpus(zp, golden, "c5"), corpus(zp, golden, "c6")
    n = min(b1.n, b2.n)
    size = max(len(b1.arena), len(b2.arena))
    d = dev()
    da = torch.zeros(size, dtype=torch.uint8, device=d)
    do = torch.zeros(n, dtype=torch.int64, device=d)
    dl = torch.zeros(n, dtype=torch.int32, device=d)
    dr = torch.zeros((n, 8), dtype=torch.uint8, device=d)
    de = torch.zeros((2, n, 16), dtype=torch.uint8, device=d)

    def load(b):
        ha, ho, hl, _ = b.device()
        da.zero_()
        da[:ha.numel()].copy_(ha)
        do.copy_(ho[:n])
        dl.copy_(hl[:n])
        zp.batch.parse_batch(da, do, dl, records=dr, ext=de)
    sel = zp.select.Select(ok=True, has=("udp",)).where("dest_port", between=(1024, 65535))
    load(b1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                        # warm up outside the capture
        zp.select.run(da, do, dl, dr, sel, want=("idx", "packed_offs"), check=False)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        s = zp.select.run(da, do, dl, dr, sel, want=("idx", "packed_offs"), check=False)
        a2, o2, l2, r2 = zp.select.gather(da, do, dl, dr, s, capacity=(n, size))
    for b in (b1, b2):
        load(b)
        g.replay()
        torch.cuda.synchronize()
        m = ref.select_mask(sel.encode(), {k: v[:n] for k, v in b.cols.items()}, b.packed[:n],
                            b.lens[:n])
        idx, po, c, total = ref.compact(m, b.lens[:n])
        assert c > 5 and s.count.tolist() == [c, total]
        assert np.array_equal(s.idx.cpu().numpy()[:c].astype(np.uint32), idx)
        assert a2.cpu().numpy()[:total].tobytes() == \
            ref.packed_bytes(b.arena, b.offs, b.lens, idx).tobytes()
        assert r2.cpu().numpy()[:c].tobytes() == b.packed[:n][idx].tobytes()
        assert np.array_equal(o2.cpu().numpy()[:c].astype(np.uint64), po)
