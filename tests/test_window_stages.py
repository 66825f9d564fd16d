"""The window-edge sweep through every stage that reads columns.

select, classify, route, the flow kernels and rewrite stage a per-lane header
window of

    wlen = min(need, len, 112 - (frame address mod 16))

bytes (zp_win.h) and take what lies past it from global memory through a
one-chunk cache; a field the window end cuts is put together byte by byte
from both sides. `need` differs by stage and by call (fx_rec_need,
zp_colrec.h): the columns kernel asks for every group, the flow kernels and
rewrite for the outer IP and L4 headers, route for the outer IP header, select
and classify for the groups their terms name. So the same frame has its
window edge elsewhere in each of them, and the sweep of tests/test_gpu_paths.py
(case_window_edge), which reaches only the columns kernel, says nothing about
the others. Here it runs through all of them, with two more inputs:

  sweep   case_window_edge's 450 frames at 16 alignments
  tails   stackgen.short_tail_families(): frames that end before `need`, so
          that wlen = len, in two arenas that differ only in the bytes between
          the frames (0x00 / 0xFF): a reader that looks past len differs
  far     the frames of tests/test_l4_far.py at 16 alignments: need = 112 and
          eth_len / inner_off read from the frame

The CPU tests compute every stage's wlen on the host from the oracle's
records and pin what makes the inputs worth running (which fields the window
end cuts, which chains lie past it). Those numbers are conditions on the
inputs; every expected output comes from the stages' CPU references
(select_ref, classify_ref, route_ref, flow_ref, flow_table_ref, rewrite_ref)
fed with the oracle's columns, byte for byte.

What the GPU tests are expected to catch, tried on an MI355X with two
mutations of zp_win.h that only give wrong values: a cached chunk that is
never refreshed (`if (h.xi == ~0u)` in hb()) fails every select, classify,
flow, flow-table and rewrite test on all three inputs and leaves route
passing, whose reads stay inside eth_len + 40 (on the far batch too: its
outer chain ends at byte 74); `hi = 0` in HdrReader::le4 fails every test
but rewrite on the far batch, where no checksum depends on a window read
(IPv6 outside, the pseudo-header's addresses and the L4 fields past byte 112).
"""
import itertools

import numpy as np
import pytest

import classify_ref as cref
import flow_table_ref as tref
import route_ref as rref
import select_ref as sref
import stackgen as sg
from rewrite_ref import WRITABLE
from test_classify import check_classify
from test_flow_table import new_table, step
from test_flows import FIVE, check_flows, opts_of
from test_gpu_paths import _cuts, get_case
from test_rewrite import random_cols, run_rewrite
from test_routes import check_route, raw_prefixes, trunc
from test_select import NAMES, SPEC, Batch, check_select

FX_WIN = 112
GROUPS = ("l3", "inner", "l4")
SUBSETS = [g for k in range(4) for g in itertools.combinations(GROUPS, k)]
INPUTS = ["sweep", "tails", "far"]


def group_of(name):
    """The column group whose header a column's getter reads (zp_select.hip
    SL_COLS_*), None for the Ethernet columns."""
    k = NAMES.index(name)
    return None if k < NAMES.index("arp_oper") else "l3" if k < NAMES.index("inner_version") \
        else "inner" if k < NAMES.index("l4_proto") else "l4"


# ---- inputs -----------------------------------------------------------------

_BUILT = {}


def _tails():
    fam = sg.short_tail_families(np.random.default_rng(4242))
    arena, offs, lens, _ = sg.place_aligned(fam["A"] + fam["B"] + fam["C"])
    return [Batch(sg.with_filler(arena, offs, lens, fill), offs, lens) for fill in (0x00, 0xFF)]


def _far():
    from test_l4_far import _cases
    arena, offs, lens, _ = sg.place_aligned([f for f, _ in _cases()])
    assert len(arena) < 64 << 20
    return [Batch(arena, offs, lens)]


def batches(zp, golden, name):
    """The input's batches (two for "tails": the two fillers), built once."""
    if name not in _BUILT:
        if name == "sweep":
            g = get_case(zp, golden, "window_edge")[0]
            b = Batch(g.arena, g.offs, g.lens)
            assert b.packed.tobytes() == g.packed.tobytes()
            _BUILT[name] = [b]
        else:
            _BUILT[name] = _tails() if name == "tails" else _far()
        for b in _BUILT[name]:
            assert (b.recs["err"] == 0).all(), name
    return _BUILT[name]


# ---- the stages' windows, on the host -----------------------------------------

def parts(zp, b):
    """Offsets and reader masks of the oracle's records, as int64 / bool arrays."""
    R, r = zp.records, b.recs
    f = r["flags"]
    has = lambda bit: (f & bit) != 0
    p = dict(hl=r["eth_len"].astype(np.int64), inner=r["inner_off"].astype(np.int64),
             l4=r["l4_off"].astype(np.int64), v4=has(R.F_IPV4), v6=has(R.F_IPV6), arp=has(R.F_ARP),
             ipip=has(R.F_IP_IN_IP), in6=has(R.F_IP_IN_IP) & has(R.F_IP_IN_IP_V6), tcp=has(R.F_TCP),
             udp=has(R.F_UDP), icmp=has(R.F_ICMPV4 | R.F_ICMPV6), ext=has(R.F_EXT),
             iext=has(R.F_INNER_EXT), ok=(r["err"] == 0) & has(R.F_ETHERNET))
    p["in4"] = p["ipip"] & ~p["in6"]
    p["anyl4"] = p["tcp"] | p["udp"] | p["icmp"]
    p["shift"] = (b.offs % 16).astype(np.int64)
    return p


def need_of(zp, b, groups):
    """fx_rec_need (zp_colrec.h) for the named groups; rewrite's own `need`
    is that of ("l3", "l4")."""
    p = parts(zp, b)
    need = np.full(b.n, 22, np.int64)
    if "l3" in groups:
        need = np.where(p["ok"], np.maximum(need, p["hl"] + 40), need)
    if "inner" in groups:
        need = np.where(p["ok"] & p["ipip"], np.maximum(need, p["inner"] + 40), need)
    if "l4" in groups:
        need = np.where(p["ok"] & p["anyl4"], np.maximum(need, p["l4"] + 20), need)
    need[zp.records.is_far(b.packed)] = FX_WIN
    return need


def wlen_of(zp, b, groups):
    return np.minimum(np.minimum(need_of(zp, b, groups), b.lens.astype(np.int64)),
                      FX_WIN - (b.offs % 16).astype(np.int64))


FLOW = ("l3", "l4")                                      # the flow kernels' and rewrite's window


def fields(zp, b):
    """{column: (offset [n], width [n], present [n])}: the frame bytes the
    column's getter reads (zp_cols.h col_values). protocol / inner_protocol of
    an IPv6 header with a chain: the chain's first two bytes, where final_nh()
    starts its walk. l4_proto comes from the record's flags and payload_off of
    UDP / ICMP from l4_off alone: they stand at the L4 header's first byte."""
    p = parts(zp, b)
    hl, inner, l4, v6, in6, tcp, udp = (p[k] for k in ("hl", "inner", "l4", "v6", "in6", "tcp", "udp"))
    ip, ipip, anyl4, every = p["v4"] | v6, p["ipip"], p["anyl4"], np.ones(b.n, bool)
    w = lambda x: np.broadcast_to(np.asarray(x, np.int64), (b.n,))
    sel = np.where
    return {
        "dest_mac": (w(0), w(6), every), "src_mac": (w(6), w(6), every),
        "ethertype": (hl - 2, w(2), every), "vlan_tci": (w(14), w(2), hl >= 18),
        "vlan_inner_tci": (w(18), w(2), hl == 22), "arp_oper": (hl + 6, w(2), p["arp"]),
        "ip_version": (hl, w(1), ip),
        "src_addr": (hl + sel(v6, 8, 12), sel(v6, 16, 4), ip),
        "dest_addr": (hl + sel(v6, 24, 16), sel(v6, 16, 4), ip),
        "protocol": (hl + sel(v6, sel(p["ext"], 40, 6), 9), sel(v6 & p["ext"], 2, 1), ip),
        "ttl": (hl + sel(v6, 7, 8), w(1), ip), "tos": (hl + sel(v6, 0, 1), sel(v6, 2, 1), ip),
        "ip_id": (hl + sel(v6, 1, 4), sel(v6, 3, 2), ip), "ip_len": (hl + sel(v6, 4, 2), w(2), ip),
        "inner_version": (inner, w(1), ipip),
        "inner_src_addr": (inner + sel(in6, 8, 12), sel(in6, 16, 4), ipip),
        "inner_dest_addr": (inner + sel(in6, 24, 16), sel(in6, 16, 4), ipip),
        "inner_protocol": (inner + sel(in6, sel(p["iext"], 40, 6), 9), sel(in6 & p["iext"], 2, 1), ipip),
        "l4_proto": (l4, w(1), anyl4),
        "src_port": (l4, w(2), tcp | udp), "dest_port": (l4 + 2, w(2), tcp | udp),
        "tcp_seq": (l4 + 4, w(4), tcp), "tcp_ack": (l4 + 8, w(4), tcp),
        "tcp_flags": (l4 + 12, w(2), tcp), "tcp_window": (l4 + 14, w(2), tcp),
        "icmp_type": (l4, w(2), p["icmp"]), "icmp_code": (l4, w(2), p["icmp"]),
        "l4_checksum": (l4 + sel(tcp, 16, sel(udp, 6, 2)), w(2), anyl4),
        "payload_off": (l4 + sel(tcp, 12, 0), sel(tcp, 2, 1), anyl4),
    }


def probes(wlen, field, most=3):
    """Up to `most` descriptors where the window end cuts the field, at
    different bytes (the first, the middle and the last of the cuts that
    occur); where it cuts none, the descriptor nearest the edge on each side.
    -> (indices, whether a cut was found)."""
    off, width, present = field
    d = wlen - off                                       # the field's bytes inside the window
    cut = present & (d >= 1) & (d < width)
    if cut.any():
        at = np.unique(d[cut])
        pick = sorted({int(at[0]), int(at[len(at) // 2]), int(at[-1])})[:most]
        return [int(np.flatnonzero(cut & (d == x))[0]) for x in pick], True
    out = []
    for side, best in ((present & (d >= width), np.argmin), (present & (d <= 0), np.argmax)):
        idx = np.flatnonzero(side)
        if len(idx):
            out.append(int(idx[best(d[idx])]))
    return out or [0], False


def value_at(b, name, i):
    return bytes(b.cols[name][i]) if SPEC[name][1] > 1 else int(b.cols[name][i])


# ---- CPU: what makes the inputs worth running ----------------------------------

def test_inputs_equal_but_for_the_filler(zp, golden):
    """The two short-tail arenas differ in no frame byte, so every reference
    (records, columns) is the same for both, and both fillers occur."""
    z, f = batches(zp, golden, "tails")
    assert np.array_equal(z.offs, f.offs) and np.array_equal(z.lens, f.lens)
    assert z.packed.tobytes() == f.packed.tobytes() and z.ext.tobytes() == f.ext.tobytes()
    for name in NAMES:
        assert np.array_equal(z.cols[name], f.cols[name]), name
    differ = z.arena != f.arena
    assert differ.sum() >= 16 * 7 and (z.arena[differ] == 0).all() and (f.arena[differ] == 0xFF).all()
    for o, n in zip(z.offs, z.lens):                     # a sample would do; all is cheap
        assert not differ[int(o):int(o) + int(n)].any()


def test_short_tails_end_inside_need(zp, golden):
    """Every short-tail descriptor has len < need for the full window (so
    wlen = len wherever 112 - shift does not end it earlier), at every
    alignment; all three families' readers occur."""
    b = batches(zp, golden, "tails")[0]
    p = parts(zp, b)
    need = need_of(zp, b, GROUPS)
    assert (b.lens < need).all()
    assert set(p["shift"].tolist()) == set(range(16))
    wl = wlen_of(zp, b, GROUPS)
    assert (wl == b.lens)[b.lens <= FX_WIN - 15].all() and (wl == b.lens).sum() >= 2000
    for k in ("udp", "icmp", "in4", "in6", "ext", "iext", "v4"):
        assert p[k].sum() >= 16, k
    assert not p["tcp"].any() and (~p["anyl4"]).sum() >= 16 * 30


def test_far_batch(zp, golden):
    b = batches(zp, golden, "far")[0]
    far = zp.records.is_far(b.packed)
    assert far.sum() >= 16 * 3 and (~far).sum() >= 16
    assert set((b.offs % 16)[far].tolist()) == set(range(16))
    assert (need_of(zp, b, ())[far] == FX_WIN).all()


def test_l4_windows_cut_the_l4_fields(zp, golden):
    """Flow / rewrite window (l3 + l4) and the L4-only window on the sweep:
    ports cut at 1 byte, tcp_seq and tcp_ack at 1, 2 and 3, the TCP flags word
    and the checksum at 1."""
    b = batches(zp, golden, "sweep")[0]
    p = parts(zp, b)
    for groups in (FLOW, ("l4",)):
        wl = wlen_of(zp, b, groups)
        for d in (4, 8):
            assert {1, 2, 3} <= _cuts(p["l4"] + d, wl, p["tcp"]), (groups, d)
        for d in (0, 2):
            assert 1 in _cuts(p["l4"] + d, wl, p["tcp"] | p["udp"]), (groups, d)
        for d in (12, 16):
            assert 1 in _cuts(p["l4"] + d, wl, p["tcp"]), (groups, d)
        assert int((p["l4"] >= wl).sum()) >= 1000        # L4 reader wholly past the window


def chain_reads(zp, b):
    """Per descriptor with an outer IPv6 chain: the frame offsets final_nh()
    reads past the fixed header (bytes 1 and 0 of every extension header)."""
    p = parts(zp, b)
    out = {}
    for i in np.flatnonzero(p["v6"] & p["ext"]):
        f = b.arena[int(b.offs[i]):int(b.offs[i]) + int(b.lens[i])]
        hl = int(p["hl"][i])
        cur, at, reads = int(f[hl + 6]), hl + 40, []
        for _ in range(bin((int(b.recs["flags"][i]) >> 12) & 63).count("1")):
            reads += [at + 1, at]
            size = 8 if cur == 44 else (int(f[at + 1]) + 2) * 4 if cur == 51 else (int(f[at + 1]) + 1) * 8
            cur, at = int(f[at]), at + size
        assert cur == int(b.recs["final_nh"][i])
        out[int(i)] = (reads, at)
    return out


def test_l3_window_leaves_the_chain_outside(zp, golden):
    """L3-only window (eth_len + 40): at least 100 IPv6 descriptors whose
    extension chain starts at or past wlen while it lies below 112 - shift
    (the columns kernel serves it from LDS, an L3-only selector from global
    memory), and for at least 16 of them final_nh()'s reads fall into two or
    more 16-B chunks, so the one-chunk cache has to refill."""
    b = batches(zp, golden, "sweep")[0]
    p = parts(zp, b)
    wl = wlen_of(zp, b, ("l3",))
    assert (wl == p["hl"] + 40).all()
    outside = refill = 0
    for i, (reads, end) in chain_reads(zp, b).items():
        if min(reads) >= wl[i] and end <= FX_WIN - p["shift"][i]:
            outside += 1
            refill += len({(x + int(p["shift"][i])) >> 4 for x in reads}) >= 2
    assert outside >= 100 and refill >= 16, (outside, refill)


def test_inner_window_cuts_the_inner_addresses(zp, golden):
    """Inner-only window: inner IPv6 src / dest cut at every byte 1..15, inner
    IPv4 src / dest at 1, 2 and 3."""
    b = batches(zp, golden, "sweep")[0]
    p = parts(zp, b)
    wl = wlen_of(zp, b, ("inner",))
    for d in (8, 24):
        assert set(range(1, 16)) <= _cuts(p["inner"] + d, wl, p["in6"]), d
    for d in (12, 16):
        assert {1, 2, 3} <= _cuts(p["inner"] + d, wl, p["in4"]), d


def test_every_subset_has_its_own_window(zp, golden):
    """The eight subsets of {l3, inner, l4} (none: need = 22) give the sweep
    at least five different windows."""
    b = batches(zp, golden, "sweep")[0]
    assert (wlen_of(zp, b, ()) == 22).all()
    assert len({wlen_of(zp, b, g).tobytes() for g in SUBSETS}) >= 5


def test_flow_flags_come_from_past_the_window(zp, golden):
    """TCP flags are part of the flow entries: some flow's flags byte comes
    from a descriptor whose l4 + 13 lies at or past the flow window's end."""
    b = batches(zp, golden, "sweep")[0]
    p = parts(zp, b)
    past = p["tcp"] & (p["l4"] + 13 >= wlen_of(zp, b, FLOW))
    assert past.sum() >= 100 and (b.cols["tcp_flags"][past] != 0).all()


REWRITE_CUT = ("src_port", "dest_port", "tcp_seq", "tcp_ack", "tcp_window")


def test_rewrite_window_cuts_the_written_fields(zp, golden):
    """The single-column rewrites of the L4 columns meet descriptors where the
    window cuts the written field (the checksum delta then needs the old value
    from both sides). The outer addresses cannot be cut: they end at eth_len +
    40 <= 62, and no window of rewrite's is shorter than 97 B unless the frame
    is; what their rewrite does meet is an L4 checksum word, which the new
    pseudo-header changes, on and past the window end."""
    b = batches(zp, golden, "sweep")[0]
    p, f = parts(zp, b), fields(zp, b)
    wl = wlen_of(zp, b, FLOW)
    for name in REWRITE_CUT:
        assert probes(wl, f[name])[1], name
    for name in ("src_addr", "dest_addr"):
        off, width, present = f[name]
        assert present.all() and (off + width <= wl).all()
    plain = ~p["ipip"]                                   # the outer addresses are the pseudo-header's
    ck = f["l4_checksum"][0]
    assert (plain & (wl - ck == 1)).any() and (plain & (ck >= wl)).sum() >= 100


def test_one_column_probes_reach_the_edge(zp, golden):
    """For the sweep, the single-column selectors of the inner and L4 groups
    have a descriptor where that selector's window cuts the column's field,
    for every column wider than one byte (inner_protocol: an inner chain
    starts where the inner-only window ends, and is probed on both sides)."""
    b = batches(zp, golden, "sweep")[0]
    f = fields(zp, b)
    for name in NAMES:
        g = group_of(name)
        if g in ("inner", "l4") and int(f[name][1].max()) > 1 and name != "inner_protocol":
            assert probes(wlen_of(zp, b, (g,)), f[name])[1], name
    wl = wlen_of(zp, b, ("inner",))
    off, _, present = f["inner_protocol"]
    assert (present & (off >= wl)).sum() >= 100 and (present & (off < wl)).sum() >= 100


# ---- rules and selectors built from a batch --------------------------------------

CANDIDATES = {"l3": ("ip_id", "ttl", "ip_len", "src_addr", "dest_addr"),
              "inner": ("inner_src_addr", "inner_dest_addr", "inner_protocol", "inner_version"),
              "l4": ("l4_checksum", "src_port", "dest_port", "icmp_code", "tcp_seq")}


def splitting_terms(zp, b, group):
    """Single terms on the group's columns that select some frames of the
    batch and leave some out, by the reference: a low bit of the value (an
    address: of its fourth, then of its third byte), then the upper half from
    the median on. A frame without the group's reader matches none of them."""
    out = []
    for name in CANDIDATES[group]:
        w = SPEC[name][1]
        if w > 1:
            bits = [bytes([0, 0, 0, 1] + [0] * (w - 4)), bytes([0, 0, 2, 0] + [0] * (w - 4))]
            kws = [dict(eq=bit, mask=bit) for bit in bits]
        else:
            kws = [dict(eq=1, mask=1)]
            d = np.unique(b.cols[name])
            if len(d) >= 3:
                kws.append(dict(between=(int(d[len(d) // 2]), int(d[-1]))))
        for kw in kws:
            m = sref.select_mask(zp.select.Select().where(name, **kw).encode(), b.cols, b.packed, b.lens)
            if m.any() and not m.all():
                out.append((name, kw))
    return out


def subset_selector(zp, b, groups):
    """One term per named group; the first combination (in CANDIDATES' order)
    whose conjunction still splits the batch."""
    for combo in itertools.product(*[splitting_terms(zp, b, g) for g in groups]):
        sel = zp.select.Select()
        for name, kw in combo:
            sel.where(name, **kw)
        m = sref.select_mask(sel.encode(), b.cols, b.packed, b.lens)
        if m.any() and not m.all():
            return sel
    raise AssertionError(f"no selector over {groups} splits the batch")


RICH = {"l3": "src_addr", "inner": "inner_src_addr", "l4": "l4_checksum"}


def subset_rules(zp, b, groups):
    """A table whose columns are exactly the groups': three frames that have
    all the groups' readers (those of the second, third and fourth greatest
    length), each by the value of one column per group, the first two with
    their length as well; then the groups' splitting terms one by one, for
    frames up to the second greatest length, so that the longest frames are
    left to the terms of the third rule or to no rule."""
    S = zp.select.Select
    full = np.all([b.cols[RICH[g]].reshape(b.n, -1).any(1) for g in groups], axis=0)
    top = np.unique(b.lens[full])[::-1][1:4]
    a, c, e = (int(np.flatnonzero(full & (b.lens == x))[0]) for x in top)
    rules = []
    for i, exact in ((a, True), (c, True), (e, False)):
        r = S(min_len=int(b.lens[i]), max_len=int(b.lens[i])) if exact else S()
        for g in groups:
            r.where(RICH[g], eq=value_at(b, RICH[g], i))
        rules.append(r)
    for k in range(2):
        for g in groups:
            terms = splitting_terms(zp, b, g)
            if k < len(terms):
                rules.append(S(max_len=int(top[0])).where(terms[k][0], **terms[k][1]))
    return rules


def column_rules(zp, b):
    """One single-column rule per column, for frames up to the second greatest
    length: the column equals its rarest non-zero value (a column with one
    value throughout: differs from it, which no frame does)."""
    S = zp.select.Select
    top = int(np.unique(b.lens)[-2])
    rules = []
    for name in NAMES:
        w = SPEC[name][1]
        v = b.cols[name].reshape(b.n, -1)
        vals, counts = np.unique(v, axis=0, return_counts=True)
        if len(vals) == 1:
            rules.append(S(max_len=top).where(name, ne=value_at(b, name, 0)))
        else:
            counts[~vals.any(1)] = b.n + 1
            i = int(np.flatnonzero((v == vals[int(np.argmin(counts))]).all(1))[0])
            rules.append(S(max_len=top).where(name, eq=value_at(b, name, i)))
    return rules


def rule_groups(rules):
    return {group_of(t[0]) for r in rules for t in r.terms} - {None}


def route_table(zp, b, by):
    """/16 and /32 of every 7th distinct IPv4 address of column `by`, /48 and
    /128 of every 7th distinct IPv6 one, in the order of their first frames.
    (Every frame stands at 16 alignments: every 7th descriptor would name every
    frame's address and leave nothing unrouted.)"""
    items = []
    for version, short, full in ((4, 16, 32), (6, 48, 128)):
        idx = np.flatnonzero(b.cols["ip_version"] == version)
        if not len(idx):
            continue
        _, first = np.unique(b.cols[by][idx], axis=0, return_index=True)
        for i in idx[np.sort(first)][::7]:
            a = bytes(b.cols[by][i])
            for length in (short, full):
                items.append((version, length, trunc(a, length), 100 + len(items)))
    return raw_prefixes(zp, items)


def test_built_rules_and_tables(zp, golden):
    """CPU: what the GPU tests below build from each input does what they rely
    on, by the references alone."""
    for name in INPUTS:
        b = batches(zp, golden, name)[0]
        for groups in SUBSETS[1:]:
            sel = subset_selector(zp, b, groups)
            assert {group_of(t[0]) for t in sel.terms} == set(groups) and len(sel.terms) == len(groups)
            rules = subset_rules(zp, b, groups)
            assert len(rules) >= 3 and rule_groups(rules) == set(groups)
            r = cref.rule_of(zp.classify.encode_rules(rules), b.cols, b.packed, b.lens)
            assert len(set(r.tolist())) >= 3 and (r == cref.RULE_NONE).any(), (name, groups)
        rules = column_rules(zp, b)
        assert [r.terms[0][0] for r in rules] == NAMES and rule_groups(rules) == set(GROUPS)
        r = cref.rule_of(zp.classify.encode_rules(rules), b.cols, b.packed, b.lens)
        assert len(set(r.tolist())) >= 3 and (r == cref.RULE_NONE).any(), name
        for by in ("src_addr", "dest_addr"):
            want = rref.value_of(route_table(zp, b, by), b.cols, b.packed, by)
            routed = set(want[want != rref.NONE].tolist())
            # the far batch has five frames with two outer headers between them
            assert (want == rref.NONE).any() and len(routed) >= (1 if name == "far" else 16), (name, by)


# ---- GPU ------------------------------------------------------------------------

def same(results):
    """The two short-tail arenas give one and the same result: each device
    output was compared with its arena's reference, and the references are
    equal, so nothing depends on the bytes between the frames."""
    for r in results[1:]:
        assert np.array_equal(r, results[0])


@pytest.mark.gpu
@pytest.mark.parametrize("name", INPUTS)
def test_select_one_column(zp, golden, name):
    """A selector with a single term on each of the 29 columns in turn: the
    smallest window that column can get. The term is `eq` on the value of a
    probe descriptor where that window cuts the column's field (the nearest
    on each side where it cuts none)."""
    S = zp.select.Select
    masks = []
    for b in batches(zp, golden, name):
        f = fields(zp, b)
        for col in NAMES:
            g = group_of(col)
            constant = len(np.unique(b.cols[col].reshape(b.n, -1), axis=0)) == 1
            for i in probes(wlen_of(zp, b, (g,) if g else ()), f[col])[0]:
                _, m = check_select(zp, b, S().where(col, eq=value_at(b, col, i)), want=("mask",))
                assert m[i], (col, i)
                assert m.all() == constant and m.any(), (col, i)
                masks.append(m)
    if name == "tails":
        same([np.concatenate(masks[:len(masks) // 2]), np.concatenate(masks[len(masks) // 2:])])


@pytest.mark.gpu
@pytest.mark.parametrize("name", INPUTS)
def test_select_group_subsets(zp, golden, name):
    """One window per non-empty subset of {l3, inner, l4}: a selector with one
    splitting term per named group; mask, idx, packed_offs and count."""
    masks = []
    for b in batches(zp, golden, name):
        for groups in SUBSETS[1:]:
            _, m = check_select(zp, b, subset_selector(zp, b, groups))
            assert m.any() and not m.all(), groups
            masks.append(m)
    if name == "tails":
        same([np.concatenate(masks[:7]), np.concatenate(masks[7:])])


@pytest.mark.gpu
@pytest.mark.parametrize("name", INPUTS)
def test_classify_group_subsets(zp, golden, name):
    got = []
    for b in batches(zp, golden, name):
        for groups in SUBSETS[1:]:
            r = check_classify(zp, b, subset_rules(zp, b, groups))
            assert len(set(r.tolist())) >= 3 and (r == cref.RULE_NONE).any(), groups
            got.append(r)
    if name == "tails":
        same([np.concatenate(got[:7]), np.concatenate(got[7:])])


@pytest.mark.gpu
@pytest.mark.parametrize("name", INPUTS)
def test_classify_every_column(zp, golden, name):
    """One single-column rule per column: the union of all three groups."""
    got = []
    for b in batches(zp, golden, name):
        rules = column_rules(zp, b)
        r = check_classify(zp, b, rules)
        assert len(set(r.tolist())) >= 3 and (r == cref.RULE_NONE).any()
        got += [r, check_classify(zp, b, rules[::-1])]
    if name == "tails":
        same([np.concatenate(got[:2]), np.concatenate(got[2:])])


@pytest.mark.gpu
@pytest.mark.parametrize("by", ["src_addr", "dest_addr"])
@pytest.mark.parametrize("name", INPUTS)
def test_route(zp, golden, name, by):
    got = []
    for b in batches(zp, golden, name):
        want, _ = check_route(zp, b, route_table(zp, b, by), by)
        routed = set(want[want != rref.NONE].tolist())
        assert (want == rref.NONE).any() and len(routed) >= (1 if name == "far" else 16)
        got.append(want)
    same(got)


@pytest.mark.gpu
@pytest.mark.parametrize("name", INPUTS)
def test_flows(zp, golden, name):
    """aggregate with key_flags 0, 15 and PORTS | PROTO: entries (keys,
    counters, TCP flags), flow_of and count."""
    got = []
    for b in batches(zp, golden, name):
        for flags in (0, 15, FIVE):
            _, (count, entries, flow_of) = check_flows(zp, b, flags)
            assert count[0] >= 2
            got.append(entries + flow_of)
    if name == "tails":
        assert got[:3] == got[3:]


@pytest.mark.gpu
@pytest.mark.parametrize("name", INPUTS)
def test_flow_table(zp, golden, name):
    """flows.Table.update over the batch in two halves."""
    got = []
    for b in batches(zp, golden, name):
        t, rt = new_table(zp, b.n), tref.Table(opts_of(FIVE, b.n))
        for lo, hi in ((0, b.n // 2), (b.n // 2, b.n)):
            count, flow_of, state = step(zp, t, rt, b, lo, hi)
        assert count[0] >= 2 and count[7] == 0
        got.append(state)
    assert got[1:] == got[:-1]


def rewrite(zp, b, names, seed):
    """run_rewrite with seeded random values; every column must have changed
    a frame if the batch has a frame with its reader."""
    cols = random_cols(np.random.default_rng(seed), b.n, names)
    _, changed, orec = run_rewrite(zp, b.arena, b.offs, b.lens, cols)
    assert (orec["err"] == 0).all()
    p = parts(zp, b)
    reader = {"vlan_tci": p["hl"] >= 18, "vlan_inner_tci": p["hl"] == 22, "src_port": p["tcp"] | p["udp"],
              "dest_port": p["tcp"] | p["udp"], "tcp_seq": p["tcp"], "tcp_ack": p["tcp"],
              "tcp_window": p["tcp"]}
    for col in names:
        assert changed[col].any() == bool(reader.get(col, p["ok"]).any()), col


@pytest.mark.gpu
@pytest.mark.parametrize("name", INPUTS)
def test_rewrite_all_columns(zp, golden, name):
    """All 14 writable columns at once, with seeded random values: the whole
    arena (the bytes between the frames too) equals rewrite_ref's, and the
    output parses to the same records without an error (run_rewrite)."""
    for b in batches(zp, golden, name):
        rewrite(zp, b, WRITABLE, 7)


@pytest.mark.gpu
@pytest.mark.parametrize("name", INPUTS)
def test_rewrite_single_columns(zp, golden, name):
    """Each writable column alone: a single write's checksum delta takes the
    field's old value from the window, from past it, or from both sides."""
    for b in batches(zp, golden, name):
        for k, col in enumerate(WRITABLE):
            rewrite(zp, b, (col,), 100 + k)
