"""The persistent flow table (zp_flow_table_init_device, zp_flow_update_device,
zp_flow_retire_device; flows.Table).

CPU: tests/flow_table_ref.py pinned on the golden packets by hand, the identity
that ties it to flow_ref.aggregate, the preconditions of the shared inputs, the
layouts and every refusal of the C ABI (they return before any HIP call).
GPU: after every call the entries, flow_of and count equal flow_table_ref
exactly. Which slot of the hash block a flow number lands in depends on the
order the hardware inserts in, so the block is checked for what it must hold
(the header, and every live number exactly once), and by the lookups of the
updates that follow.

The two-piece tests cut the shared batch at n / 4: at n / 2 only 14 flows
begin in the second piece, at n / 4 there are 24 (asserted below).
"""
import os
import re

import numpy as np
import pytest

import flow_ref as ref
import flow_table_ref as tref
import select_ref
from test_columns import pack
from test_flows import FIVE, flow_frames, mixed, opts_of
from test_select import Batch, dev, to_dev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 0xA5
FIN, SYN, RST = 1, 2, 4
SENT = -1431655766                                       # 0xAAAAAAAA as int32


def cut(b):
    return b.n // 4


def pieces(n, k):
    e = [n * j // k for j in range(k + 1)]
    return list(zip(e[:-1], e[1:]))


def ref_run(b, opts, parts, mask=None):
    """The reference table after the given pieces -> (table, [(flow_of, count)])."""
    t = tref.Table(opts)
    return t, [t.update(*tref.piece(b, lo, hi), None if mask is None else mask[lo:hi]) for lo, hi in parts]


# ---- CPU ------------------------------------------------------------------------

def test_reference_on_the_golden_packets(zp, golden):
    """The fixtures in two batches, [0, 2) and [2, 24): fixture 1 founds flow 0
    in update 0 and fixture 2 (the same 5-tuple, another VLAN) hits it in
    update 1; every other keyed fixture is admitted in update 1."""
    frames = [bytes.fromhex(fx["bytes"]) for fx in golden["fixtures"]]
    b = Batch(*pack(frames))
    assert b.n == 24
    t = tref.Table(opts_of(FIVE, 100))
    fo, cnt = t.update(*tref.piece(b, 0, 2))
    assert list(fo) == [ref.NONE, 0] and cnt == [1, 1, 1, 64, 0, 0, 0, 0]
    fo, cnt = t.update(*tref.piece(b, 2, 24))
    total = int(b.lens.sum()) - 54 - 42 - 54 - 54 - 64     # the rejected fixtures 0, 15-18
    assert cnt == [18, 17, 18, total - 64, 0, 0, 1, 0]
    assert fo[0] == 0 and list(fo[1:5]) == [1, 2, 3, 4]
    assert all(fo[i - 2] == ref.NONE for i in (15, 16, 17, 18))
    st = t.states()
    assert (st["first_epoch"][0], st["last_epoch"][0], st["packets_flags"][0], st["bytes"][0]) == (0, 1, 2, 128)
    assert (st["first_epoch"][1:] == 1).all() and (st["last_epoch"][1:] == 1).all()
    assert st["packets_flags"][4] == 1 | 0x12 << 56         # the SYN-ACK of fixture 6
    assert int(st["key"]["src_port"][0]) == 1234 and int(st["key"]["dest_port"][0]) == 5678
    # a third update of all fixtures into a table of 18 + 0: every flow hit, nothing new
    fo, cnt = t.update(*tref.piece(b, 0, 24))
    assert cnt[:2] == [18, 0] and cnt[6] == 2 and int(t.states()["packets_flags"][0] & tref.PACKETS_MASK) == 4
    # retire: nothing is idle (all seen in update 2); SYN retires flow 4 and renumbers those behind it
    gone, remap, rc = t.retire(1, 0)
    assert rc == [18, 0] and len(gone) == 0 and list(remap) == list(range(18))
    gone, remap, rc = t.retire(tref.IDLE_NEVER, SYN)
    assert remap[4] == ref.NONE and rc[0] + rc[1] == 18 and rc[1] == len(gone) >= 1
    assert list(remap[:4]) == [0, 1, 2, 3] and remap[5] in (4, ref.NONE)
    assert (gone["packets_flags"] >> np.uint64(56)).astype(int).tolist()[0] & SYN
    gone, remap, rc = t.retire(0, 0)
    assert rc[0] == 0 and t.states().size == 0
    # capacity 2: the first two new keys by first frame are admitted, the rest refused
    t = tref.Table(opts_of(FIVE, 2))
    fo, cnt = t.update(*tref.piece(b, 0, 24))
    assert cnt == [2, 2, 19, total, 16, 16, 0, 0]
    assert list(fo[:5]) == [ref.NONE, 0, 0, 1, ref.NONE]


@pytest.mark.parametrize("k", [1, 2, 3, 7, 40])
def test_reference_splits_equal_aggregate(zp, golden, k):
    """For any split into consecutive pieces, with capacity >= F and no
    retire, the table equals flow_ref.aggregate over the whole batch."""
    b = mixed(zp, golden)
    for flags in (FIVE, FIVE | ref.BIDIR | ref.VLAN, 0):
        opts = opts_of(flags, b.n)
        wfo, went, wcnt = ref.aggregate(b.cols, b.packed, b.lens, opts)
        rng = np.random.default_rng(k)
        edges = [0] + sorted(rng.choice(np.arange(1, b.n), k - 1, replace=False).tolist()) + [b.n]
        t, res = ref_run(b, opts, list(zip(edges[:-1], edges[1:])))
        st = t.states()
        assert st["key"].tobytes() == went["key"].tobytes()
        assert np.array_equal(st["packets_flags"] & np.uint64(tref.PACKETS_MASK), went["packets"])
        assert np.array_equal(st["bytes"], went["bytes"])
        assert np.array_equal((st["packets_flags"] >> np.uint64(56)).astype(np.uint8), went["tcp_flags"])
        assert np.array_equal(np.concatenate([fo for fo, _ in res]), wfo)
        assert res[-1][1][0] == wcnt[0] and sum(c[2] for _, c in res) == wcnt[1]
        assert sum(c[3] for _, c in res) == wcnt[2] and sum(c[1] for _, c in res) == wcnt[0]


RETIRE_PARTS = [(0, 1000), (1000, 1100), (1100, 1160)]    # flows end up at three ages
RETIRE_CASES = {"idle0": (0, 0), "idle1": (1, 0), "idle2": (2, 0), "flags": (None, FIN | RST),
                "both": (2, FIN | RST), "none": (None, 0), "none_idle": (3, 0), "all": (0, FIN | RST)}


def overflow_setup(b):
    """(capacity, k): the table holds the first piece's flows and k more."""
    t, _ = ref_run(b, opts_of(FIVE, b.n), [(0, cut(b))])
    return len(t.entries) + 3, 3


def test_shared_input_preconditions(zp, golden):
    b = mixed(zp, golden)
    h = cut(b)
    wfo, _, _ = ref.aggregate(b.cols, b.packed, b.lens, opts_of(FIVE, b.n))
    first, second = set(wfo[:h].tolist()) - {ref.NONE}, set(wfo[h:].tolist()) - {ref.NONE}
    assert len(first & second) >= 100 and len(second - first) >= 20
    # the overflow case
    cap, k = overflow_setup(b)
    t, res = ref_run(b, opts_of(FIVE, cap), [(0, h), (h, b.n)])
    fo, cnt = res[1]
    assert cnt[0] == cap and cnt[1] == k and cnt[4] > 0 and cnt[5] > cnt[4]
    known = fo[fo != ref.NONE]
    assert (known < cap - k).sum() > 100, "established flows still counted"
    refused_at = np.flatnonzero((fo == ref.NONE) & ref.keyed(b.packed[h:]))
    assert len(refused_at) == cnt[5]
    assert np.flatnonzero((fo >= cap - k) & (fo != ref.NONE)).max() > refused_at.min(), \
        "a frame of an admitted new flow behind a refused frame"
    # the retire cases: some retired, some kept, and a retired key comes back
    for name, (idle, any_) in RETIRE_CASES.items():
        t, _ = ref_run(b, opts_of(FIVE, b.n), RETIRE_PARTS)
        f = len(t.entries)
        old = [e["key"] for e in t.entries]
        gone, remap, rc = t.retire(tref.IDLE_NEVER if idle is None else idle, any_)
        if name.startswith("none"):
            assert rc == [f, 0]
        elif name in ("all", "idle0"):
            assert rc == [0, f]
        else:
            assert rc[0] >= 20 and rc[1] >= 20, (name, rc)
        if rc[1]:
            fo, cnt = t.update(*tref.piece(b, 1160, b.n))
            back = [t.number[k_] for j, k_ in enumerate(old) if remap[j] == ref.NONE and k_ in t.number]
            assert len(back) >= 10 and min(back) >= rc[0], name
            assert all(t.entries[j]["first_epoch"] == 3 for j in back)
    ages = 2 - ref_run(b, opts_of(FIVE, b.n), RETIRE_PARTS)[0].states()["last_epoch"]
    assert all((ages == a).sum() >= 20 for a in (0, 1, 2))


def test_layouts_and_constants(zp):
    fl = zp.flows
    assert fl.STATE_DTYPE.itemsize == 64 and fl.STATE_DTYPE == tref.STATE_DTYPE
    assert [fl.STATE_DTYPE.fields[k][1] for k in ("key", "first_epoch", "last_epoch", "packets_flags", "bytes")] \
        == [0, 40, 44, 48, 56]
    hdr = open(os.path.join(ROOT, "include", "zero_packet.h")).read()
    assert re.search(r"#define ZP_FLOW_STATE_PACKETS\(e\)\s+\(\(e\)\.packets_flags & 0x00FFFFFFFFFFFFFFull\)", hdr)
    assert re.search(r"#define ZP_FLOW_STATE_TCP_FLAGS\(e\)\s+\(\(uint8_t\)\(\(e\)\.packets_flags >> 56\)\)", hdr)
    assert int(re.search(r"#define ZP_FLOW_IDLE_NEVER\s+0x([0-9A-F]+)u", hdr).group(1), 16) == fl.IDLE_NEVER \
        == tref.IDLE_NEVER
    assert int(re.search(r"#define ZP_ABI_VERSION (\d+)", hdr).group(1)) == 6
    e = np.zeros(2, fl.STATE_DTYPE)
    e["packets_flags"] = [5 | 0x12 << 56, (1 << 56) - 1 | 0xFF << 56]
    assert fl.state_packets(e).tolist() == [5, (1 << 56) - 1] == (e["packets_flags"] & np.uint64(tref.PACKETS_MASK)).tolist()
    assert fl.state_tcp_flags(e).tolist() == [0x12, 0xFF]
    # sizeof: the C++ program's static_assert (test_flow_table_cpp) holds the compiler to 64 too
    lib = zp._lib.hip()
    tb, ub, rb = lib.zp_flow_table_bytes, lib.zp_flow_update_scratch_bytes, lib.zp_flow_retire_scratch_bytes
    sizes = (1, 2, 31, 32, 33, 63, 64, 65, 1000, 4096, 262144, 262145, (1 << 24) + 5, 1 << 28, 1 << 30)
    for a, c in zip(sizes[:-1], sizes[1:]):
        assert tb(a) <= tb(c) and ub(a) <= ub(c) and rb(a) <= rb(c)
    for m in sizes:
        assert 64 + 4 * 2 * m <= tb(m) <= 16 * m + 512 and (tb(m) - 64) % 4 == 0
        s = (tb(m) - 64) // 4
        assert s & (s - 1) == 0 and s >= 64 and s >= 2 * m and (s == 64 or s < 4 * m)
        assert 48 * m < ub(m) <= 96 * m + 4096 and ub(m) == lib.zp_flow_scratch_bytes(m, m)
        assert 64 * m < rb(m) <= 72 * m + 4096
    assert ub(0) > 0 and rb(1) > 0


def test_refusals_touch_no_device(zp):
    """Every refusal returns negative with its cause named, before any HIP
    call: the pointers given are never dereferenced."""
    lib, fl = zp._lib.hip(), zp.flows
    P = 4096                                              # a non-null "device pointer"
    ok = fl.encode_opts(FIVE, 100)
    tbytes = int(lib.zp_flow_table_bytes(100))
    big = int(lib.zp_flow_update_scratch_bytes(1000))
    rbig = int(lib.zp_flow_retire_scratch_bytes(100))

    def update(enc, arena=P, offs=P, lens=P, recs=P, n=1000, mask=None, table=P, ntable=tbytes, flows=P,
               flow_of=P, count=P, scratch=P, nscratch=big):
        return lib.zp_flow_update_device(arena, offs, lens, recs, n,
                                         enc.ctypes.data if enc is not None else None, mask, table, ntable,
                                         flows, flow_of, count, scratch, nscratch, None)

    def retire(enc, table=P, ntable=tbytes, flows=P, max_idle=1, tcp_any=0, retired=P, remap=P, count=P,
               scratch=P, nscratch=rbig):
        return lib.zp_flow_retire_device(enc.ctypes.data if enc is not None else None, table, ntable, flows,
                                         max_idle, tcp_any, retired, remap, count, scratch, nscratch, None)

    def init(enc, table=P, ntable=tbytes):
        return lib.zp_flow_table_init_device(table, ntable, enc.ctypes.data if enc is not None else None,
                                             None)

    def refused(fn, what, *a, **kw):
        assert fn(*a, **kw) < 0, what
        msg = lib.zp_last_error().decode()
        assert msg.startswith({update: "zp_flow_update_device: ", retire: "zp_flow_retire_device: ",
                               init: "zp_flow_table_init_device: "}[fn]) and what in msg, (what, msg)

    def with_(**kw):
        e = ok.copy()
        for k, v in kw.items():
            e[k] = v
        return e
    for fn in (update, retire, init):                     # what the three calls share
        refused(fn, "null opts", None)
        refused(fn, "unknown key_flags", with_(key_flags=16))
        refused(fn, "unknown key_flags", with_(key_flags=0x80000001))
        refused(fn, "pad", with_(pad=1))
        refused(fn, "max_flows", with_(max_flows=0))
        refused(fn, "2^30", with_(max_flows=(1 << 30) + 1), ntable=1 << 40)
        refused(fn, "null table", ok, table=None)
        refused(fn, "table_bytes", ok, ntable=tbytes - 1)
        refused(fn, "misaligned", ok, table=P + 4)
    # aggregate's list, and what update adds to it
    refused(update, "null records", ok, recs=None)
    refused(update, "null lens", ok, lens=None)
    refused(update, "null arena", ok, arena=None)
    refused(update, "null offs", ok, offs=None)
    refused(update, "null flows", ok, flows=None)
    refused(update, "null count", ok, count=None)
    refused(update, "scratch", ok, scratch=None)
    refused(update, "scratch", ok, nscratch=big - 1)
    refused(update, "2^31", ok, n=1 << 31, nscratch=1 << 62)
    refused(update, "2^31", ok, n=1 << 32, nscratch=1 << 62)
    refused(update, "misaligned", ok, flows=P + 8)
    refused(update, "misaligned", ok, flow_of=P + 2)
    refused(update, "misaligned", ok, count=P + 4)
    refused(update, "misaligned", ok, mask=P + 1)
    refused(retire, "null flows", ok, flows=None)
    refused(retire, "null count", ok, count=None)
    refused(retire, "scratch", ok, scratch=None)
    refused(retire, "scratch", ok, nscratch=rbig - 1)
    refused(retire, "tcp_any", ok, tcp_any=0x100)
    refused(retire, "misaligned", ok, retired=P + 8)
    refused(retire, "misaligned", ok, remap=P + 2)
    refused(retire, "misaligned", ok, count=P + 4)


def test_facade_argument_checks(zp):
    fl = zp.flows
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fl.Table(10, "cpu")
    with pytest.raises(ValueError):
        fl.Table(0, "cuda:0")
    assert "SYNCHRONISATION" in fl.Table.to_numpy.__doc__
    assert fl.Table.update.__defaults__[:2] == (None, ("flow_of",))
    assert fl.Table.retire.__defaults__[:3] == (None, 0, ("retired", "remap"))


# ---- GPU ------------------------------------------------------------------------

def new_table(zp, cap, flags=FIVE, hash_mask=None):
    """A Table over guard-filled tensors, two entries longer than the capacity."""
    import torch
    nb = int(zp._lib.hip().zp_flow_table_bytes(cap))
    out = {"table": torch.full((nb + 64,), GUARD, dtype=torch.uint8, device=dev()),
           "flows": torch.full((cap + 2, 64), GUARD, dtype=torch.uint8, device=dev())}
    t = zp.flows.Table(cap, dev(), ports=bool(flags & ref.PORTS), proto=bool(flags & ref.PROTO),
                       vlan=bool(flags & ref.VLAN), bidir=bool(flags & ref.BIDIR), hash_mask=hash_mask, out=out)
    t.nbytes = nb
    return t


def check_state(zp, t, rt):
    """The device table against the reference one: entries, header, slots."""
    raw = t.table.cpu().numpy()
    flows = t.flows.cpu().numpy()
    cap, f = t.max_flows, len(rt.entries)
    assert (flows[cap:] == GUARD).all(), "flows written past max_flows"
    assert (raw[t.nbytes:] == GUARD).all(), "the table block written past its size"
    hdr = raw[:64].view("<u8")
    assert (int(hdr[2]), int(hdr[3])) == (f, rt.epoch) and (hdr[4:] == 0).all()
    want = rt.states()
    got = flows[:f].reshape(-1).view(tref.STATE_DTYPE)
    assert got.tobytes() == want.tobytes(), [
        (i, got[i], want[i]) for i in range(f) if got[i].tobytes() != want[i].tobytes()][:2]
    slots = raw[64:t.nbytes].view("<u4")
    assert np.array_equal(np.sort(slots[slots != 0xFFFFFFFF]), np.arange(f)), "every flow once in the slots"
    return flows[:f].tobytes()


def step(zp, t, rt, b, lo, hi, mask=None, dmask=None, scratch_fill=None, **kw):
    """One update of [lo, hi) on the device and in the reference; everything compared."""
    import torch
    da, do, dl, dr = b.device()
    n = hi - lo
    out = {"count": torch.full((8,), -1, dtype=torch.int64, device=dev()),
           "flow_of": torch.full((n + 8,), SENT, dtype=torch.int32, device=dev())}
    if scratch_fill is not None:
        nb = int(zp._lib.hip().zp_flow_update_scratch_bytes(n))
        out["scratch"] = torch.full((nb,), scratch_fill, dtype=torch.uint8, device=dev())
    if mask is not None and dmask is None:
        dmask, = to_dev(select_ref.mask_words(mask))
    u = t.update(da, do[lo:hi], dl[lo:hi], dr[lo:hi], mask=dmask, out=out, **kw)
    wfo, wcnt = rt.update(*tref.piece(b, lo, hi), mask)
    count = [int(v) for v in u.count.tolist()]
    fo = u.flow_of.cpu().numpy().view(np.uint32)
    assert (fo[n:] == 0xAAAAAAAA).all(), "flow_of written past n"
    assert count == wcnt, (count, wcnt)
    assert np.array_equal(fo[:n], wfo), np.flatnonzero(fo[:n] != wfo)[:8]
    return count, fo[:n].tobytes(), check_state(zp, t, rt)


def do_retire(zp, t, rt, max_idle=None, tcp_any=0):
    import torch
    cap, f_old = t.max_flows, len(rt.entries)
    out = {"count": torch.full((2,), -1, dtype=torch.int64, device=dev()),
           "retired": torch.full((cap + 2, 64), GUARD, dtype=torch.uint8, device=dev()),
           "remap": torch.full((cap + 8,), SENT, dtype=torch.int32, device=dev())}
    before = t.flows.cpu().numpy().copy()
    r = t.retire(max_idle, tcp_any, out=out)
    wgone, wremap, wcnt = rt.retire(tref.IDLE_NEVER if max_idle is None else max_idle, tcp_any)
    assert [int(v) for v in r.count.tolist()] == wcnt
    gone, remap = r.retired.cpu().numpy(), r.remap.cpu().numpy().view(np.uint32)
    assert gone[:wcnt[1]].tobytes() == wgone.tobytes() and (gone[wcnt[1]:] == GUARD).all()
    assert np.array_equal(remap[:f_old], wremap) and (remap[f_old:] == 0xAAAAAAAA).all()
    keep = wremap != ref.NONE
    after = t.flows.cpu().numpy()
    assert after[:wcnt[0]].tobytes() == before[:f_old][keep].tobytes(), "survivors byte for byte, in order"
    assert np.array_equal(after[wcnt[0]:], before[wcnt[0]:]), "entries at and past F' are left as they are"
    return wcnt, gone[:wcnt[1]].tobytes(), remap[:f_old].tobytes(), check_state(zp, t, rt)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 2, 7])
def test_pieces(zp, golden, k):
    b = mixed(zp, golden)
    cap = b.n
    t, rt = new_table(zp, cap), tref.Table(opts_of(FIVE, cap))
    for lo, hi in ([(0, cut(b)), (cut(b), b.n)] if k == 2 else pieces(b.n, k)):
        step(zp, t, rt, b, lo, hi)
    da, do, dl, dr = b.device()
    ent = zp.flows.to_numpy(zp.flows.aggregate(da, do, dl, dr))
    got = t.to_numpy()
    assert len(got) == len(ent) >= 150 and got["key"].tobytes() == ent["key"].tobytes()
    assert np.array_equal(zp.flows.state_packets(got), ent["packets"])
    assert np.array_equal(got["bytes"], ent["bytes"])
    assert np.array_equal(zp.flows.state_tcp_flags(got), ent["tcp_flags"])
    assert (got["last_epoch"] <= k - 1).all() and (got["first_epoch"] <= got["last_epoch"]).all()


@pytest.mark.gpu
def test_same_batch_twice(zp, golden):
    b = mixed(zp, golden)
    t, rt = new_table(zp, b.n), tref.Table(opts_of(FIVE, b.n))
    c0, fo0, _ = step(zp, t, rt, b, 0, b.n)
    one = t.to_numpy()
    c1, fo1, _ = step(zp, t, rt, b, 0, b.n)
    two = t.to_numpy()
    assert c1[0] == c0[0] and c1[1] == 0 and fo1 == fo0 and c1[2:4] == c0[2:4]
    assert two["key"].tobytes() == one["key"].tobytes() and (two["last_epoch"] == 1).all()
    assert np.array_equal(zp.flows.state_packets(two), 2 * zp.flows.state_packets(one))
    assert np.array_equal(two["bytes"], 2 * one["bytes"]) and (two["first_epoch"] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("flags", range(16))
def test_key_flags(zp, golden, flags):
    b = mixed(zp, golden)
    t, rt = new_table(zp, b.n, flags), tref.Table(opts_of(flags, b.n))
    step(zp, t, rt, b, 0, cut(b))
    c, _, _ = step(zp, t, rt, b, cut(b), b.n)
    assert c[1] > 0 and c[2] > c[1]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257])
def test_batch_sizes(zp, golden, n):
    """n frames as the second update after a first of 300: hits and new keys
    share waves and tiles. n == 0: the epoch advances and count is exact."""
    b = mixed(zp, golden)
    t, rt = new_table(zp, b.n), tref.Table(opts_of(FIVE, b.n))
    step(zp, t, rt, b, 0, 300)
    c, _, _ = step(zp, t, rt, b, 300, 300 + n)
    if n >= 63:
        assert c[1] >= 1 and c[2] - c[1] >= 10, "new keys and hits"
    if n == 0:
        assert c == [c[0], 0, 0, 0, 0, 0, 1, 0] and t.header() == (c[0], 2)
    step(zp, t, rt, b, 300 + n, 700)


@pytest.mark.gpu
@pytest.mark.parametrize("hash_mask", [0, 1, 7])
def test_forced_collisions(zp, golden, hash_mask):
    b = mixed(zp, golden)

    def run(hm):
        t, rt = new_table(zp, b.n, hash_mask=hm), tref.Table(opts_of(FIVE, b.n))
        got = [step(zp, t, rt, b, lo, hi) for lo, hi in RETIRE_PARTS]
        got.append(do_retire(zp, t, rt, 1, FIN))
        got.append(step(zp, t, rt, b, 1160, b.n))
        return got
    assert run(hash_mask) == run(None)


@pytest.mark.gpu
def test_capacity(zp, golden):
    b = mixed(zp, golden)
    h = cut(b)
    f = ref_run(b, opts_of(FIVE, b.n), [(0, b.n)])[0].states().size
    t, rt = new_table(zp, f), tref.Table(opts_of(FIVE, f))          # exactly F: no refusals
    step(zp, t, rt, b, 0, h)
    c, _, _ = step(zp, t, rt, b, h, b.n)
    assert c[0] == f and c[4] == c[5] == 0
    cap, k = overflow_setup(b)
    t, rt = new_table(zp, cap), tref.Table(opts_of(FIVE, cap))
    step(zp, t, rt, b, 0, h)
    c, fo, _ = step(zp, t, rt, b, h, b.n)
    assert c[:2] == [cap, k] and c[4] > 0 and c[5] > c[4]
    refused, was = c[4], (np.frombuffer(fo, np.uint32) == ref.NONE) & ref.keyed(b.packed[h:])
    c, _, _ = step(zp, t, rt, b, 0, b.n)                             # on the full table: still exact
    assert c[:2] == [cap, 0] and c[4] == refused
    wc, _, _, _ = do_retire(zp, t, rt, None, FIN | RST)              # makes room
    assert wc[1] > refused, "room for every refused key"
    c, _, _ = step(zp, t, rt, b, h, b.n, mask=was)                   # the frames refused before
    assert c[1] == refused and c[4] == 0 and c[2] == was.sum(), "the keys refused before are admitted"
    step(zp, t, rt, b, 0, b.n)


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(RETIRE_CASES))
def test_retire(zp, golden, case):
    b = mixed(zp, golden)
    idle, any_ = RETIRE_CASES[case]
    t, rt = new_table(zp, b.n), tref.Table(opts_of(FIVE, b.n))
    for lo, hi in RETIRE_PARTS:
        step(zp, t, rt, b, lo, hi)
    wc, _, _, _ = do_retire(zp, t, rt, idle, any_)
    c, _, _ = step(zp, t, rt, b, 1160, b.n)                # lookups after the rebuild; retired keys return
    got = t.to_numpy()
    assert (got["first_epoch"][wc[0]:] == 3).all() and c[1] == len(got) - wc[0]
    assert c[2] - c[1] > 0 or wc[0] == 0, "survivors are found again"
    step(zp, t, rt, b, 0, 300)


@pytest.mark.gpu
def test_scan_boundary(zp):
    """Past a scan workgroup's span: the rank scan's second level runs in the
    update (all new), the second update is all hits, and a retire over more
    than ZP_SELECT_SCAN_FRAMES entries splits the flows by a TCP flag."""
    import torch
    n = zp.select.SCAN_FRAMES + 300
    da, do, dl = zp.batch.generate("c2", n, first=77, device=dev())
    dr, _ = zp.batch.parse_batch(da, do, dl)
    torch.cuda.synchronize()
    b = Batch(da.cpu().numpy(), do.cpu().numpy(), dl.cpu().numpy())
    b.d = [da, do, dl, dr]
    assert dr.cpu().numpy().tobytes() == b.packed.tobytes()
    t, rt = new_table(zp, n), tref.Table(opts_of(FIVE, n))
    c, _, _ = step(zp, t, rt, b, 0, n)
    f = c[0]
    assert f == c[1] > 1000
    c, _, _ = step(zp, t, rt, b, 0, n)
    assert c[:2] == [f, 0]
    assert f > zp.select.SCAN_FRAMES, "retire's second scan level has flows to rank"
    # The generated c2 frames carry no TCP flags, so no tcp_any splits these
    # flows (the bit that splits them best is still passed). A third update
    # of two frames in three leaves every third flow one update older, and
    # max_idle = 1 retires those, across every tile.
    flags = zp.flows.state_tcp_flags(rt.states())
    bit = max((1 << k for k in range(8)), key=lambda m: min(int((flags & m != 0).sum()), int((flags & m == 0).sum())))
    m = np.arange(n) % 3 != 0
    c, _, _ = step(zp, t, rt, b, 0, n, mask=m)
    assert c[:3] == [f, 0, int(m.sum())]
    wc, _, remap, _ = do_retire(zp, t, rt, 1, bit)
    remap = np.frombuffer(remap, np.uint32)
    assert wc[0] > 100000 and wc[1] > 80000
    assert (remap[zp.select.SCAN_FRAMES:] != ref.NONE).any() and (remap[zp.select.SCAN_FRAMES:] == ref.NONE).any()
    step(zp, t, rt, b, n - 600, n)


@pytest.mark.gpu
def test_mismatched_or_uninitialised_table(zp, golden):
    import torch
    b = mixed(zp, golden)
    da, do, dl, dr = b.device()
    t, rt = new_table(zp, b.n), tref.Table(opts_of(FIVE, b.n))
    step(zp, t, rt, b, 0, 500)
    other = [zp.flows.encode_opts(FIVE | ref.VLAN, b.n), zp.flows.encode_opts(FIVE, b.n - 1),
             zp.flows.encode_opts(FIVE, b.n, 7), None]
    for enc in other:
        if enc is None:                                    # never initialised
            t.table.fill_(GUARD)
            enc = t.opts
        tb, fb = t.table.clone(), t.flows.clone()
        out = {"count": torch.full((8,), -1, dtype=torch.int64, device=dev()),
               "flow_of": torch.full((b.n,), SENT, dtype=torch.int32, device=dev())}
        u = t.update(da, do, dl, dr, out=out, opts=enc)
        assert u.count.tolist() == [-1] * 7 + [1]
        assert torch.equal(t.table, tb) and torch.equal(t.flows, fb) and (u.flow_of == SENT).all()
        u = t.update(da, do[:0], dl[:0], dr[:0], out=out, opts=enc)       # n == 0 checks too
        assert u.count.tolist() == [-1] * 7 + [1] and torch.equal(t.table, tb)
        out = {"count": torch.full((2,), 5, dtype=torch.int64, device=dev()),
               "retired": torch.full((b.n, 64), GUARD, dtype=torch.uint8, device=dev()),
               "remap": torch.full((b.n,), SENT, dtype=torch.int32, device=dev())}
        r = t.retire(0, 0xFF, out=out, opts=enc)
        assert r.count.tolist() == [5, -1]
        assert torch.equal(t.table, tb) and torch.equal(t.flows, fb)
        assert (r.retired == GUARD).all() and (r.remap == SENT).all()


@pytest.mark.gpu
def test_dirty_scratch_and_determinism(zp, golden):
    b = mixed(zp, golden)
    lib = zp._lib.hip()

    def run(fill=None):
        t, rt = new_table(zp, b.n, FIVE | ref.BIDIR), tref.Table(opts_of(FIVE | ref.BIDIR, b.n))
        return [step(zp, t, rt, b, lo, hi, scratch_fill=fill) for lo, hi in ((0, cut(b)), (cut(b), b.n))]
    first = run()
    assert run() == first
    for fill in (0xFF, 0x00, 0x5A):
        assert run(fill) == first, fill
    was = lib.zp__flow_combine(0)
    try:
        assert run() == first
    finally:
        lib.zp__flow_combine(was)


@pytest.mark.gpu
def test_one_flow_and_all_distinct(zp, golden):
    """The two ends of the in-wave combining, each updated twice."""
    f = flow_frames(zp, golden, 1, seed=3)[0]
    for b in (Batch(*pack([f] * 1500)), Batch(*pack(flow_frames(zp, golden, 1500, seed=4)))):
        for on in (1, 0):
            was = zp._lib.hip().zp__flow_combine(on)
            try:
                t, rt = new_table(zp, b.n), tref.Table(opts_of(FIVE, b.n))
                step(zp, t, rt, b, 0, 700)
                c, _, _ = step(zp, t, rt, b, 300, b.n)
                assert c[0] in (1, 1500)
            finally:
                zp._lib.hip().zp__flow_combine(was)


@pytest.mark.gpu
def test_graph_replay(zp, golden):
    """update(check=False) captured once and replayed twice from a fresh init:
    the epoch lives on the device, so the second replay is update 1."""
    import torch
    b = mixed(zp, golden)
    da, do, dl, dr = b.device()
    t = new_table(zp, b.n, FIVE | ref.BIDIR)
    out = {"count": torch.zeros(8, dtype=torch.int64, device=dev()),
           "flow_of": torch.zeros(b.n, dtype=torch.int32, device=dev()),
           "scratch": torch.zeros(int(zp._lib.hip().zp_flow_update_scratch_bytes(b.n)), dtype=torch.uint8,
                                  device=dev())}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                          # warm up outside the capture
        t.update(da, do, dl, dr, out=out, check=False)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        u = t.update(da, do, dl, dr, out=out, check=False)
    t.init()
    rt = tref.Table(opts_of(FIVE | ref.BIDIR, b.n))
    for e in range(2):
        for v in out.values():
            v.fill_(0x33)
        g.replay()
        torch.cuda.synchronize()
        wfo, wcnt = rt.update(b.cols, b.packed, b.lens)
        assert [int(v) for v in u.count.tolist()] == wcnt and wcnt[6] == e
        assert np.array_equal(u.flow_of.cpu().numpy().view(np.uint32), wfo)
        check_state(zp, t, rt)


@pytest.mark.gpu
def test_layouts(zp, golden):
    """The test_flows.test_layouts batch (odd offsets, gaps, shuffled
    descriptors, far-L4 frames) in two pieces, then a mask from select."""
    from test_l4_far import _cases
    from wrapframes import parse_fixtures
    b0 = mixed(zp, golden)
    frames = [b0.arena[int(o):int(o) + int(l)].tobytes() for o, l in zip(b0.offs, b0.lens)][:600]
    far = [f for f, _ in _cases()][:2] + [parse_fixtures()["ffffffff"][0]]
    frames = frames[:300] + far + frames[300:] + far
    arena, offs, lens = pack(frames)
    assert (offs % 2 == 1).any() and (np.diff(offs.astype(np.int64)) > lens[:-1]).all()
    p = np.random.default_rng(1).permutation(len(offs))
    b = Batch(arena, offs[p], lens[p])
    assert (b.recs["l4_off"] > 0x3FFFF).any()
    for flags in (FIVE, FIVE | ref.BIDIR | ref.VLAN):
        t, rt = new_table(zp, b.n, flags), tref.Table(opts_of(flags, b.n))
        step(zp, t, rt, b, 0, 250)
        step(zp, t, rt, b, 250, b.n)
        # the UDP frames of the second piece only, by the mask select writes for that piece
        da, do, dl, dr = b.device()
        sel = zp.select.Select(ok=True).where("l4_proto", eq=17)
        s = zp.select.run(da, do[250:], dl[250:], dr[250:], sel, want=("mask",))
        m = select_ref.select_mask(sel.encode(), *tref.piece(b, 250, b.n))
        assert 30 < m.sum() < ref.keyed(b.packed[250:]).sum()
        c, _, _ = step(zp, t, rt, b, 250, b.n, mask=m, dmask=s.mask)
        assert c[2] == m.sum()
