"""Classify (zp_classify_compile, zp_classify_device, classify.py).

CPU: tests/classify_ref.py pinned on the golden packets by hand-written
expectations, the compiled table (deterministic, every refusal), every
refusal of zp_classify_device (they return before any HIP call) and the
facade's constants.
GPU: rule_of, hits and the mask words equal classify_ref as whole arrays, in
sentinel-filled buffers 64 entries longer than the batch.
"""
import os
import re

import numpy as np
import pytest

import classify_ref as cref
import oracle as orc
import select_ref as sref
from test_columns import pack
from test_select import (Batch, both_sides, corpus, dev, golden_batch, synthetic, threshold,
                         to_dev)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [c[0] for c in orc.COLUMN_SPEC]
SPEC = {name: (dt, w) for name, dt, w in orc.COLUMN_SPEC}
BYTE_ARRAYS = [name for name, dt, w in orc.COLUMN_SPEC if w > 1]
NONE = cref.RULE_NONE


# ---- CPU: the reference pinned by hand --------------------------------------

def test_reference_on_the_golden_packets(zp, golden):
    S, C = zp.select.Select, zp.classify
    arena, offs, lens, recs, ext, cols, packed = golden_batch(golden)
    rules = [S(has=("tcp",)), S().where("dest_port", eq=5678),
             S(has=("tcp",)).where("dest_port", eq=43424), S(ok=False), S(ok=True)]
    tcp, p5678, bad = [6, 7, 8, 12, 23], [1, 2], [0, 15, 16, 17, 18]
    want = np.full(24, 4, np.uint32)
    want[tcp], want[p5678], want[bad] = 0, 1, 3
    got = cref.rule_of(C.encode_rules(rules), cols, packed, lens)
    assert got.tolist() == want.tolist()
    h = cref.hits(got, lens, 5)
    assert h["packets"].tolist() == [5, 2, 0, 5, 12, 0]          # rule 2 is shadowed; no frame unmatched
    assert h["bytes"][0] == 804 and h["bytes"].sum() == lens.sum()
    assert h["bytes"][1] == int(lens[1]) + int(lens[2]) and h["bytes"][2] == 0
    # the same rules reversed: every accepted frame goes to the rule that is now first
    rev = cref.rule_of(C.encode_rules(rules[::-1]), cols, packed, lens)
    want = np.zeros(24, np.uint32)
    want[bad] = 1
    assert rev.tolist() == want.tolist()
    assert cref.hits(rev, lens, 5)["packets"].tolist() == [19, 5, 0, 0, 0, 0]
    # without a catch-all, frames fall to "no rule"
    some = cref.rule_of(C.encode_rules(rules[:3]), cols, packed, lens)
    assert sorted(np.flatnonzero(some == NONE)) == sorted(set(range(24)) - set(tcp) - set(p5678))
    assert cref.hits(some, lens, 3)["packets"].tolist() == [5, 2, 0, 17]
    # mask words: any rule / a set with the no-rule bit / the empty set
    assert cref.mask_words(some, 3)[0] == sum(1 << i for i in tcp + p5678)
    assert cref.mask_words(some, 3, [1, NONE])[0] == sum(1 << i for i in range(24) if i not in tcp)
    assert cref.mask_words(some, 3, [])[0] == 0


def test_constants_and_accept_words(zp):
    C = zp.classify
    hdr = open(os.path.join(ROOT, "include", "zero_packet.h")).read()
    assert int(re.search(r"#define ZP_CLASSIFY_MAX_RULES (\d+)", hdr).group(1)) == C.MAX_RULES
    assert int(re.search(r"#define ZP_RULE_NONE (0x[0-9A-Fa-f]+)u", hdr).group(1), 16) == C.RULE_NONE
    assert re.search(r"#define ZP_ABI_VERSION 6\b", hdr)
    assert C.HITS_DTYPE.itemsize == 16 and C.HITS_DTYPE == cref.HITS_DTYPE
    assert C.accept_words([0, 63, C.RULE_NONE], 63).tolist() == [(1 << 0) | (1 << 63)] and \
        C.accept_words([64], 64).tolist() == [0, 1] and \
        C.accept_words([C.RULE_NONE], 64).tolist() == [0, 1] and \
        C.accept_words([], 256).tolist() == [0] * 5
    with pytest.raises(ValueError):
        C.accept_words([4], 3)
    with pytest.raises(TypeError):
        C.encode_rules(["tcp"])


# ---- CPU: compile -----------------------------------------------------------

def five_tuple(zp, k):
    S = zp.select.Select
    return (S(ok=True).where("src_addr", prefix=f"10.{k}.0.0/16").where("dest_port", between=(k, k + 100))
            .where("l4_proto", eq=6).where("ip_version", eq=4))


def test_compile_is_deterministic_and_sized(zp):
    C, lib = zp.classify, zp._lib.hip()
    sizes = [int(lib.zp_classify_table_bytes(r)) for r in range(1, C.MAX_RULES + 1)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0 and sizes[0] % 8 == 0
    assert lib.zp_classify_table_bytes(0) == 0 and lib.zp_classify_table_bytes(C.MAX_RULES + 1) == 0
    assert max(sizes) < 1 << 20
    rules = C.encode_rules([five_tuple(zp, k) for k in range(40)])
    nb = sizes[39]
    # the same input into differently filled buffers: the same bytes, nothing behind them
    outs = []
    for fill in (0x00, 0xA5):
        t = np.full(nb // 8 + 8, fill * 0x0101010101010101, np.uint64)
        assert lib.zp_classify_compile(rules.ctypes.data, 40, t.ctypes.data, nb + 64) == 1
        assert (t[nb // 8:] == fill * 0x0101010101010101).all(), "written past table_bytes(nrules)"
        outs.append(t[:nb // 8].tobytes())
    assert outs[0] == outs[1]
    host, frames = C.compile_rules(rules)
    assert frames and host.tobytes() == outs[0]
    # other rules, other bytes; a record-only table says so
    other = rules.copy()
    other[7]["min_len"] = 1
    assert C.compile_rules(other)[0].tobytes() != outs[0]
    S = zp.select.Select
    host, frames = C.compile_rules(C.encode_rules([S(ok=True), S(has=("tcp",), min_len=60)]))
    assert not frames
    # the header records whether any rule has terms and the union of the terms' columns
    w = C.compile_rules(rules)[0].view("<u4")
    union = sum(1 << NAMES.index(c) for c in ("src_addr", "dest_port", "l4_proto", "ip_version"))
    assert w[2] == 40 and w[3] & 1 and w[4] == union
    assert not host.view("<u4")[3] & 1 and host.view("<u4")[4] == 0
    # forty rules share l4_proto == 6 and ip_version == 4: stored once each
    assert w[6] == 40 + 40 + 1 + 1 and w[5] == 1


def test_compile_refusals(zp):
    C, lib, sl = zp.classify, zp._lib.hip(), zp.select
    S = sl.Select
    good = C.encode_rules([S(ok=True).where("ttl", eq=3) for _ in range(5)])
    nb = int(lib.zp_classify_table_bytes(5))
    buf = np.full(nb // 8, 0x5A5A5A5A5A5A5A5A, np.uint64)

    def refused(what, rules, nrules=5, nbytes=nb, table=buf):
        rc = lib.zp_classify_compile(rules.ctypes.data if rules is not None else None, nrules,
                                     table.ctypes.data if table is not None else None, nbytes)
        assert rc < 0, what
        msg = lib.zp_last_error().decode()
        assert "zp_classify_compile" in msg and what in msg, (what, msg)
        assert (buf == 0x5A5A5A5A5A5A5A5A).all(), "the table was touched by a refused compile"
    for bad_rule in (0, 3, 4):
        e = good.copy(); e[bad_rule]["nterms"] = 9
        refused(f"rule {bad_rule}: more than ZP_SELECT_MAX_TERMS", e)
        e = good.copy(); e[bad_rule]["terms"][0]["col"] = len(NAMES)
        refused(f"rule {bad_rule}: term 0: column {len(NAMES)} out of range", e)
        e = good.copy(); e[bad_rule]["terms"][0]["pad"][4] = 1
        refused(f"rule {bad_rule}: term 0: pad", e)
        e = good.copy(); e[bad_rule]["terms"][0]["op"] = 4
        refused(f"rule {bad_rule}: term 0: unknown op", e)
        for name in BYTE_ARRAYS:
            for op in (sl.RANGE, sl.NOT_RANGE):
                e = good.copy()
                e[bad_rule]["terms"][0]["col"], e[bad_rule]["terms"][0]["op"] = NAMES.index(name), op
                refused(f"rule {bad_rule}: term 0: RANGE on byte-array", e)
    # a bad second term of a later rule is named too
    e = C.encode_rules([S(), S().where("ttl", eq=1).where("tos", eq=2)])
    e[1]["terms"][1]["op"] = 7
    refused("rule 1: term 1: unknown op", e, nrules=2)
    refused("nrules 0", good, nrules=0)
    refused("nrules 257", good, nrules=257, nbytes=1 << 30)
    refused("table_bytes", good, nbytes=nb - 1)
    refused("null", None)
    refused("null", good, table=None)
    assert lib.zp_classify_compile(good.ctypes.data, 5, buf.ctypes.data, nb) == 1
    with pytest.raises(ValueError):
        C.compile_rules(np.zeros(0, sl.SELECT_DTYPE))


def test_device_refusals_touch_no_device(zp):
    """Every refusal returns negative with its cause named, before any HIP
    call: the pointers given are never dereferenced."""
    lib = zp._lib.hip()
    P = 4096                                             # a non-null "device pointer"
    nb = int(lib.zp_classify_table_bytes(7))
    acc = np.zeros(1, np.uint64)

    def call(arena=P, offs=P, lens=P, recs=P, n=1000, table=P, nbytes=nb, nrules=7, accept=None,
             rule_of=P, hits=P, mask=P, status=P):
        return lib.zp_classify_device(arena, offs, lens, recs, n, table, nbytes, nrules,
                                      accept, rule_of, hits, mask, status, None)

    def refused(what, **kw):
        assert call(**kw) < 0, what
        msg = lib.zp_last_error().decode()
        assert "zp_classify_device" in msg and what in msg, (what, msg)
    refused("null records", recs=None)
    refused("null table", table=None)
    refused("null status", status=None)
    refused("nrules", nrules=0)
    refused("nrules", nrules=257, nbytes=1 << 30)
    refused("table_bytes", nbytes=nb - 1)
    refused("table_bytes", nrules=8)                     # sized for 7 rules
    refused("2^32", n=1 << 32)
    refused("misaligned", table=P + 4)
    refused("misaligned", hits=P + 4)
    refused("misaligned", mask=P + 4)
    refused("misaligned", status=P + 4)
    refused("misaligned", rule_of=P + 2)
    refused("hits need lens", lens=None, arena=None, offs=None)
    refused("needs arena, offs and lens", arena=None)
    refused("needs arena, offs and lens", offs=None)
    refused("needs arena, offs and lens", lens=None, hits=None)
    refused("null records", recs=None, accept=acc.ctypes.data)


# ---- GPU --------------------------------------------------------------------

SENT_R, SENT_M, PAD = -7, -9, 64
START = 1000                                             # hits start from non-zero values


def start_hits(nrules):
    """nrules + 1 pairs {START + k, 3 * (START + k)} and PAD sentinel pairs behind."""
    h = np.zeros((nrules + 1 + PAD, 2), np.int64)
    h[:, 0] = START + np.arange(len(h))
    h[:, 1] = 3 * h[:, 0]
    return h


def classify(zp, b, table, want=("rule_of", "hits", "mask"), accept=None, hits=None, use_arena=True,
             use_lens=True, **kw):
    """table.run into sentinel-filled buffers PAD entries longer than needed
    -> (Classified, rule_of, hits, mask as numpy; None where not wanted),
    asserting that nothing past the batch was written."""
    import torch
    da, do, dl, dr = b.device()
    n, nr = b.n, table.nrules
    out = {"rule_of": torch.full((n + PAD,), SENT_R, dtype=torch.int32, device=dev()),
           "mask": torch.full(((n + 63) // 64 + PAD,), SENT_M, dtype=torch.int64, device=dev()),
           "hits": hits if hits is not None else to_dev(start_hits(nr))[0],
           "status": torch.full((1,), -1, dtype=torch.int64, device=dev())}
    c = table.run(da if use_arena else None, do if use_arena else None, dl if use_lens else None,
                  dr, want=want, accept=accept, out=out, **kw)
    torch.cuda.synchronize()
    assert int(c.status[0]) == 0
    r = h = m = None
    if "rule_of" in want:
        r = c.rule_of.cpu().numpy()
        assert (r[n:] == SENT_R).all(), "rule_of written past n"
        r = r[:n].view(np.uint32)
    else:
        assert c.rule_of is None and (out["rule_of"] == SENT_R).all()
    if "hits" in want:
        h = c.hits.cpu().numpy()
        assert np.array_equal(h[nr + 1:], start_hits(nr)[nr + 1:]), "hits written past nrules + 1"
        h = h[:nr + 1]
    if "mask" in want:
        m = c.mask.cpu().numpy()
        assert (m[(n + 63) // 64:] == SENT_M).all(), "mask written past ceil(n / 64)"
        m = m[:(n + 63) // 64].view(np.uint64)
    else:
        assert c.mask is None and (out["mask"] == SENT_M).all()
    return c, r, h, m


def hits_plus(start, ref_hits):
    """start (int64 pairs) + reference hits, wrapping as the 64-bit adds do."""
    out = start[:len(ref_hits)].copy().view(np.uint64)
    out[:, 0] += ref_hits["packets"]
    out[:, 1] += ref_hits["bytes"]
    return out.view(np.int64)


def check_classify(zp, b, rules, accept=None, use_arena=True, reference=None):
    """Runs the table on the device and compares everything with classify_ref;
    returns the reference rule_of."""
    C = zp.classify
    table = C.RuleTable(rules, dev())
    assert table.needs_frames == any(r.terms for r in rules)
    want = reference if reference is not None else \
        cref.rule_of(table.rules, b.cols, b.packed, b.lens)
    _, r, h, m = classify(zp, b, table, accept=accept, use_arena=use_arena)
    assert np.array_equal(r, want), np.flatnonzero(r != want)[:8]
    wh = hits_plus(start_hits(table.nrules), cref.hits(want, b.lens, table.nrules))
    assert np.array_equal(h, wh), (h[:8], wh[:8])
    assert np.array_equal(m, cref.mask_words(want, table.nrules, accept))
    return want


SIZES = [1, 63, 64, 65, 255, 256, 257]


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_sizes_record_only(zp, n):
    """Record-only tables on hand-set records (a lens entry of 0xFFFFFFF0
    among them), run with arena=None, offs=None."""
    S = zp.select.Select
    b = synthetic(n, n)
    for name, rules in (("none", [S(has=("arp",))]), ("all", [S(has=("ethernet",))]),
                        ("first", [S(has=("tcp",))]), ("last", [S(has=("udp",))]),
                        ("mixed", [S(has=("arp",)), S(has=("tcp",)), S(has=("udp",)),
                                   S(has=("icmpv4",), max_len=40000), S(has=("icmpv6",))])):
        r = check_classify(zp, b, rules, use_arena=False)
        if name in ("first", "last"):
            assert list(np.flatnonzero(r == 0)) == [0 if name == "first" else n - 1]
        elif name in ("none", "all"):
            assert (r == (NONE if name == "none" else 0)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_sizes_with_terms(zp, n):
    S = zp.select.Select
    b = Batch(*zp.batch.generate_host("c3", n, first=5))
    assert (b.recs["err"] == 0).all() and (b.cols["l4_proto"] != 0).all()

    def only(i):
        c = b.cols
        return (S().where("l4_checksum", eq=int(c["l4_checksum"][i]))
                .where("ip_id", eq=int(c["ip_id"][i])).where("src_port", eq=int(c["src_port"][i]))
                .where("src_addr", eq=bytes(c["src_addr"][i])))
    for name, rules in (("none", [S().where("ip_version", eq=0)]),
                        ("all", [S().where("ttl", between=(0, 255))]),
                        ("first", [only(0)]), ("last", [only(n - 1)]),
                        ("mixed", [S().where("ip_version", eq=0), only(n - 1), only(0),
                                   S().where("l4_checksum", eq=1, mask=1)])):
        r = check_classify(zp, b, rules)
        if name in ("first", "last"):
            assert list(np.flatnonzero(r == 0)) == [0 if name == "first" else n - 1]
        elif name in ("none", "all"):
            assert (r == (NONE if name == "none" else 0)).all()


RULE_COUNTS = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256]
_c3 = {}


def c3_batch(zp):
    if "b" not in _c3:
        _c3["b"] = Batch(*zp.batch.generate_host("c3", 4096, first=5))
    return _c3["b"]


def disjoint(zp, R):
    return [zp.select.Select().where("l4_checksum", eq=r, mask=0xFF) for r in range(R)]


def nested(zp, R):
    return [zp.select.Select().where("src_port", between=((R - 1 - r) * (65536 // R), 65535))
            for r in range(R)]


def test_rule_count_inputs(zp):
    """CPU: the 4,096 c3 frames carry what the two rule families rely on."""
    b = c3_batch(zp)
    low = np.bincount(b.cols["l4_checksum"] & 0xFF, minlength=256)
    assert low.min() >= 7, "every low byte of l4_checksum occurs"
    assert len(np.unique(b.cols["src_port"] >> 8)) == 256
    icmp = b.cols["l4_proto"] == 1
    assert icmp.any() and (b.cols["src_port"][icmp] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("R", RULE_COUNTS)
def test_rule_counts_disjoint(zp, R):
    """Rule r: l4_checksum & 0xFF == r. Every rule is hit; below 256 rules the
    other low bytes fall to the unmatched entry."""
    b = c3_batch(zp)
    rules = disjoint(zp, R)
    want = cref.rule_of(zp.classify.encode_rules(rules), b.cols, b.packed, b.lens)
    assert set(want.tolist()) >= set(range(R)), "inputs: every rule index must occur"
    assert (want == NONE).any() == (R < 256)
    check_classify(zp, b, rules, reference=want)


@pytest.mark.gpu
@pytest.mark.parametrize("R", RULE_COUNTS)
def test_rule_counts_nested(zp, R):
    """Rule r: src_port in [(R-1-r) * (65536 // R), 65535]: a frame matches
    every rule from its own on, the lowest must win."""
    b = c3_batch(zp)
    rules = nested(zp, R)
    want = cref.rule_of(zp.classify.encode_rules(rules), b.cols, b.packed, b.lens)
    assert len(set(want.tolist())) >= min(R, 200), "inputs: the rules must be spread over"
    assert (want[b.cols["l4_proto"] == 1] == R - 1).all()         # port 0: only the last rule
    check_classify(zp, b, rules, reference=want)


def priority_rules(zp):
    S = zp.select.Select
    return [S(ok=True).where("l4_proto", eq=6), S(ok=True).where("ip_version", eq=4),
            S(ok=True, has=("udp",)), S(ok=False), S().where("dest_port", between=(1, 65535)),
            S(ok=True, min_len=100)]


@pytest.mark.gpu
def test_priority(zp, golden):
    S, C = zp.select.Select, zp.classify
    b = corpus(zp, golden)
    rules = priority_rules(zp)
    fwd = check_classify(zp, b, rules)
    rev = check_classify(zp, b, rules[::-1])
    assert not np.array_equal(fwd, rev) and len(set(fwd.tolist())) >= 5
    # two identical adjacent rules: the second gets nothing
    twice = [rules[1], rules[0], rules[0], rules[3]]
    r = check_classify(zp, b, twice)
    assert (r == 1).any() and not (r == 2).any()
    # forty rules share one term and differ in the second
    forty = [S().where("l4_proto", eq=6).where("l4_checksum", eq=k, mask=0x3F) for k in range(40)]
    r = check_classify(zp, b, forty + [S().where("l4_proto", eq=6)])
    assert len(set(r.tolist())) >= 30 and (r == 40).any() and (r == NONE).any()
    assert C.compile_rules(C.encode_rules(forty))[0].view("<u4")[6] == 41


def column_rules(zp, b):
    """One rule per column of orc.COLUMN_SPEC (a range for scalars, a masked
    equality for byte arrays) and `ok=False & ttl == 0` behind them."""
    S = zp.select.Select
    rules = []
    for name in NAMES:
        dt, w = SPEC[name]
        t, top = threshold(b.cols[name])
        if w > 1:
            m = bytes([0xFF] * (w - 1) + [0xF0])
            rules.append(S().where(name, eq=bytes(x & y for x, y in zip(bytes(t), m)), mask=m))
        else:
            rules.append(S().where(name, between=(int(t[0]), int(top[0]))))
    return rules + [S(ok=False).where("ttl", eq=0)]


def test_every_column_inputs(zp, golden):
    """CPU: each of the 30 rules matches some frame of the corpus and misses some."""
    b = corpus(zp, golden)
    rules = column_rules(zp, b)
    assert len(rules) == 30 == len(NAMES) + 1
    for r in rules:
        both_sides(sref.select_mask(r.encode(), b.cols, b.packed, b.lens))


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["forward", "reversed"])
def test_every_column(zp, golden, order):
    b = corpus(zp, golden)
    rules = column_rules(zp, b)
    r = check_classify(zp, b, rules if order == "forward" else rules[::-1])
    bad = b.recs["err"] != 0
    # error records read all zero: they match `ok=False & ttl == 0` unless an earlier rule takes 0
    assert (r[bad] != NONE).all() and len(set(r.tolist())) >= 8


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", ["c4", "c5", "c6"])
def test_rules_of_eight_terms(zp, golden, cfg):
    b = corpus(zp, golden, cfg)
    S = zp.select.Select
    okm = b.recs["err"] == 0
    ttl, _ = threshold(b.cols["ttl"][okm])
    i = int(np.flatnonzero(okm & (b.cols["l4_proto"] != 0))[5])
    c = b.cols
    eight = (S(ok=True).where("src_addr", eq=bytes(c["src_addr"][i]))
             .where("dest_addr", eq=bytes(c["dest_addr"][i]))
             .where("src_port", eq=int(c["src_port"][i])).where("dest_port", eq=int(c["dest_port"][i]))
             .where("l4_proto", eq=int(c["l4_proto"][i])).where("ip_version", eq=int(c["ip_version"][i]))
             .where("ttl", between=(0, 255)).where("src_mac", mac=bytes(c["src_mac"][i])))
    rules = [eight,
             S(ok=True).where("src_addr", eq=bytes(c["src_addr"][i])).where("l4_proto", eq=int(c["l4_proto"][i])),
             S(has=("ipv6",), min_len=80).where("ttl", between=(int(ttl[0]), 255)),
             S(ok=False).where("ttl", eq=0),
             S(ok=True, max_len=120).where("l4_proto", eq=17).where("src_port", between=(1, 40000)),
             S(ok=True, any_of=("tcp", "udp"), lacks=("ip_in_ip",), min_len=70),
             S(ok=True).where("ip_version", ne=0)]
    r = check_classify(zp, b, rules)
    assert r[i] == 0 and len(set(r.tolist()) - {NONE}) >= 5
    check_classify(zp, b, rules[::-1])


@pytest.mark.gpu
def test_far_l4_and_past_the_window(zp, golden):
    """The far-L4 frames of tests/test_l4_far.py and c4 frames whose L4 header
    lies past the staged window, in a table whose columns reach the L4 header."""
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
    c = b.cols
    rules = []
    for i in list(range(len(far))) + [len(far), len(far) + 1]:
        rules.append(S().where("l4_checksum", eq=int(c["l4_checksum"][i]))
                     .where("l4_proto", eq=int(c["l4_proto"][i]))
                     .where("payload_off", eq=int(c["payload_off"][i]))
                     .where("src_port", eq=int(c["src_port"][i]))
                     .where("inner_src_addr", eq=bytes(c["inner_src_addr"][i])))
    rules += [S().where("tcp_seq", ne=0), S().where("icmp_type", ne=0), S().where("inner_version", ne=0)]
    r = check_classify(zp, b, rules)
    for k in range(len(far) + 2):
        assert r[k] <= k, "a frame matches the rule made from it, or an equal earlier one"
    check_classify(zp, b, rules[::-1])


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["gaps", "reverse", "shuffled", "dup"])
def test_layouts(zp, golden, layout):
    from test_gpu_parity import layout_batch
    b0 = corpus(zp, golden)
    frames = [b0.arena[int(o):int(o) + int(l)].tobytes() for o, l in zip(b0.offs, b0.lens)][:900]
    b = Batch(*layout_batch(frames, layout))
    S = zp.select.Select
    port, _ = threshold(b.cols["dest_port"])
    r = check_classify(zp, b, [S(ok=True).where("dest_port", between=(int(port[0]), 65535)),
                               S().where("ip_version", eq=6).where("ttl", outside=(0, 32)),
                               S(has=("udp",), min_len=80),
                               S().where("src_addr", ne=bytes(16))])
    assert len(set(r.tolist())) == 5


# ---- GPU: counters ----------------------------------------------------------

@pytest.mark.gpu
def test_counters_accumulate_over_batches(zp, golden):
    b1, b2 = corpus(zp, golden, "c5"), corpus(zp, golden, "c6")
    table = zp.classify.RuleTable(priority_rules(zp), dev())
    nr = table.nrules
    hits, = to_dev(start_hits(nr))
    want = start_hits(nr)[:nr + 1]
    for b in (b1, b2):
        ref = cref.rule_of(table.rules, b.cols, b.packed, b.lens)
        _, r, h, _ = classify(zp, b, table, hits=hits)
        assert np.array_equal(r, ref)
        want = hits_plus(want, cref.hits(ref, b.lens, nr))
        assert np.array_equal(h, want)
    # the table's own tensor, through hits_numpy(): from zero
    table.run(*b1.device())
    ref = cref.rule_of(table.rules, b1.cols, b1.packed, b1.lens)
    assert table.hits_numpy().tobytes() == cref.hits(ref, b1.lens, nr).tobytes()
    table.reset_hits()
    assert not table.hits_numpy()["packets"].any()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [257, 70000])
def test_hot_rule(zp, n):
    """Every frame matches rule 0: whole waves reduce before they touch the
    workgroup's histogram; the byte sum passes 2^32."""
    S = zp.select.Select
    b = synthetic(n, n + 1)
    assert int(b.lens.astype(np.uint64).sum()) > 1 << 32
    r = check_classify(zp, b, [S(has=("ethernet",)), S()], use_arena=False)
    assert (r == 0).all()
    if n == 257:                                         # and through the term kernel
        b = Batch(*zp.batch.generate_host("c3", n, first=5))
        r = check_classify(zp, b, [S().where("ttl", between=(0, 255)), S()])
        assert (r == 0).all()


@pytest.mark.gpu
def test_rule_of_alone(zp, golden):
    """hits NULL, mask NULL: the same rule_of, and neither buffer is touched;
    a record-only table without lens."""
    b = corpus(zp, golden, "c5")
    table = zp.classify.RuleTable(priority_rules(zp), dev())
    ref = cref.rule_of(table.rules, b.cols, b.packed, b.lens)
    for want in (("rule_of",), ("rule_of", "mask"), ("hits",), ("mask",), ()):
        c, r, h, m = classify(zp, b, table, want=want)
        if r is not None:
            assert np.array_equal(r, ref)
        if h is not None:
            assert np.array_equal(h, hits_plus(start_hits(table.nrules), cref.hits(ref, b.lens, table.nrules)))
        if m is not None:
            assert np.array_equal(m, cref.mask_words(ref, table.nrules))
    assert not table.hits.any(), "the table's own counters were not asked for"
    S = zp.select.Select
    rec = zp.classify.RuleTable([S(has=("tcp",)), S(ok=False), S(has=("ipv6",))], dev())
    ref = cref.rule_of(rec.rules, None, b.packed, None)
    _, r, _, m = classify(zp, b, rec, want=("rule_of", "mask"), use_arena=False, use_lens=False)
    assert np.array_equal(r, ref) and np.array_equal(m, cref.mask_words(ref, 3))
    assert len(set(ref.tolist())) == 4


@pytest.mark.gpu
def test_record_only_on_fuzzed_batches(zp, golden):
    S = zp.select.Select
    for cfg in ("c5", "c6"):
        b = corpus(zp, golden, cfg)
        errs = np.unique(b.recs["err"])
        rules = [S(has=("ipv4", "udp"), min_len=100), S(has=("tcp",)), S(ok=True, lacks=("tcp", "udp")),
                 S(any_of=("icmpv4", "icmpv6", "arp")), S(ok=True, min_len=64, max_len=200)]
        rules += [S(err=int(e)) for e in errs if e] + [S(max_len=99), S()]
        r = check_classify(zp, b, rules, use_arena=False)
        assert len(set(r.tolist())) >= 6 and not (r == NONE).any()
        check_classify(zp, b, rules[-2::-1], use_arena=False)


# ---- GPU: accept and mask ---------------------------------------------------

@pytest.mark.gpu
def test_accept_sets(zp, golden):
    b = corpus(zp, golden)
    rules = priority_rules(zp)[:3]
    for accept in (None, [1, NONE], [], [0, 2], [NONE]):
        r = check_classify(zp, b, rules, accept=accept)
    assert (r == NONE).any() and len(set(r.tolist())) == 4
    # 65 rules: the no-rule bit is bit 65 % 64 of the second word
    b = c3_batch(zp)
    for accept in ([64], [NONE], [63, 64, NONE]):
        check_classify(zp, b, disjoint(zp, 65), accept=accept)


@pytest.mark.gpu
def test_mask_feeds_the_flow_table(zp, golden):
    import flow_ref
    from test_flows import FIVE, mixed, opts_of, read, run
    S = zp.select.Select
    b = mixed(zp, golden)
    table = zp.classify.RuleTable([S(ok=True).where("l4_proto", eq=17),
                                   S(ok=True).where("ip_version", eq=6),
                                   S(ok=True).where("l4_proto", eq=6)], dev())
    ref = cref.rule_of(table.rules, b.cols, b.packed, b.lens)
    c = table.run(*b.device(), want=("mask",), accept=[0, 2])
    m = cref.accepted(ref, 3, [0, 2])
    assert 100 < m.sum() < flow_ref.keyed(b.packed).sum()
    t = run(zp, b, mask=c.mask)
    count, flows, fo = read(t, b.n, b.n)
    wfo, went, wcnt = flow_ref.aggregate(b.cols, b.packed, b.lens, opts_of(FIVE, b.n), m)
    assert count == wcnt and np.array_equal(fo, wfo)
    assert flows[:wcnt[0]].tobytes() == went.tobytes()
    assert set(went["key"]["l4_proto"].tolist()) == {6, 17}


# ---- GPU: status ------------------------------------------------------------

def raw(zp, b, table_t, nrules, frames=True, lens=True, n=None):
    """zp_classify_device into sentinel buffers -> (rc, status, rule_of, hits, mask)."""
    import torch
    da, do, dl, dr = b.device()
    n = b.n if n is None else n
    rule_of = torch.full((n + PAD,), SENT_R, dtype=torch.int32, device=dev())
    mask = torch.full(((n + 63) // 64 + PAD,), SENT_M, dtype=torch.int64, device=dev())
    hits, = to_dev(start_hits(nrules))
    status = torch.full((1,), -1, dtype=torch.int64, device=dev())
    rc = zp._lib.hip().zp_classify_device(
        da.data_ptr() if frames else None, do.data_ptr() if frames else None,
        dl.data_ptr() if lens else None, dr.data_ptr(), n, table_t.data_ptr(), table_t.numel(),
        nrules, None, rule_of.data_ptr(), hits.data_ptr() if lens else None, mask.data_ptr(),
        status.data_ptr(), None)
    torch.cuda.synchronize()
    return rc, int(status[0]), rule_of.cpu().numpy(), hits.cpu().numpy(), mask.cpu().numpy()


@pytest.mark.gpu
def test_status_refuses_a_wrong_table(zp, golden):
    """The kernel checks the header before anything else: a table compiled for
    another rule count, a zeroed one, and a claim the header contradicts give
    status 1 and leave every output as it was."""
    import torch
    S = zp.select.Select
    b = corpus(zp, golden, "c5")
    t3 = zp.classify.RuleTable(priority_rules(zp)[:3], dev())
    bounded = zp.classify.RuleTable([S(min_len=80), S()], dev())
    assert not bounded.needs_frames

    def untouched(res, nrules):
        rc, status, r, h, m = res
        assert rc == 0 and status == 1
        assert (r == SENT_R).all() and (m == SENT_M).all()
        assert np.array_equal(h, start_hits(nrules))
    untouched(raw(zp, b, t3.table, 2), 2)                          # compiled for 3 rules
    untouched(raw(zp, b, torch.zeros_like(t3.table), 3), 3)        # never written
    untouched(raw(zp, b, t3.table, 3, frames=False), 3)            # "record-only", but it has terms
    untouched(raw(zp, b, bounded.table, 2, frames=False, lens=False), 2)   # bounds need lens
    rc, status, r, h, m = raw(zp, b, t3.table, 3)                  # and the right call goes through
    ref = cref.rule_of(t3.rules, b.cols, b.packed, b.lens)
    assert rc == 0 and status == 0 and np.array_equal(r[:b.n].view(np.uint32), ref)
    assert (r[b.n:] == SENT_R).all()
    # the facade raises on it
    t3.nrules = 2
    with pytest.raises(RuntimeError, match="status 1"):
        t3.run(*b.device(), want=("rule_of",))
    # n == 0 writes status only
    rc, status, r, h, m = raw(zp, b, bounded.table, 2, n=0)
    assert rc == 0 and status == 0 and (r == SENT_R).all() and (m == SENT_M).all()
    assert np.array_equal(h, start_hits(2))


# ---- GPU: graph -------------------------------------------------------------

@pytest.mark.gpu
def test_enqueue_only_in_a_graph(zp, golden):
    """run(check=False) captured once on one stream and replayed twice: hits
    is twice the reference, rule_of the same."""
    import torch
    b = corpus(zp, golden, "c5")
    da, do, dl, dr = b.device()
    table = zp.classify.RuleTable(priority_rules(zp), dev())
    out = {"rule_of": torch.full((b.n,), SENT_R, dtype=torch.int32, device=dev()),
           "mask": torch.zeros((b.n + 63) // 64, dtype=torch.int64, device=dev()),
           "status": torch.full((1,), -1, dtype=torch.int64, device=dev())}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                        # warm up outside the capture
        table.run(da, do, dl, dr, out=out, check=False)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    table.reset_hits()
    out["rule_of"].fill_(SENT_R)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        c = table.run(da, do, dl, dr, out=out, check=False)
    ref = cref.rule_of(table.rules, b.cols, b.packed, b.lens)
    h1 = cref.hits(ref, b.lens, table.nrules)
    for k in (1, 2):
        g.replay()
        torch.cuda.synchronize()
        h = table.hits_numpy()
        assert np.array_equal(h["packets"], k * h1["packets"]) and \
            np.array_equal(h["bytes"], k * h1["bytes"])
        assert np.array_equal(c.rule_of.cpu().numpy().view(np.uint32), ref)
        assert int(c.status[0]) == 0
        assert np.array_equal(c.mask.cpu().numpy().view(np.uint64), cref.mask_words(ref, table.nrules))
