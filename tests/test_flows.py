"""Flow table (zp_flow_aggregate_device, flows.py).

CPU: tests/flow_ref.py pinned on the golden packets by hand-written
expectations, the struct layouts and constants, every refusal of the C ABI
(they return before any HIP call) and the facade's argument checks.
GPU: every result equals flow_ref exactly: flow_of as an array, the first F
entries byte for byte, count as four integers. Each test first asserts, on
the CPU, that its batch has the property it is there for.
"""
import os
import random
import re

import numpy as np
import pytest

import flow_ref as ref
import oracle as orc
import select_ref
from fuzzfix import repair
from test_columns import pack
from test_select import Batch, dev, to_dev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIVE = ref.PORTS | ref.PROTO
GUARD = 0xA5
F_TCP, F_UDP = 1 << 6, 1 << 7


# ---- frames -----------------------------------------------------------------

def edit(frame, rec, src=None, dst=None, sport=None, dport=None, swap=False):
    """The accepted frame with other outer addresses / L4 ports (or the two
    endpoints swapped), its checksums refilled."""
    f = bytearray(frame)
    hl = int(rec["eth_len"])
    v6 = bool(int(rec["flags"]) & ref.F_IPV6)
    a, w = (hl + 8, 16) if v6 else (hl + 12, 4)
    p = int(rec["l4_off"]) if int(rec["flags"]) & (F_TCP | F_UDP) else None
    if swap:
        f[a:a + w], f[a + w:a + 2 * w] = f[a + w:a + 2 * w], f[a:a + w]
        if p is not None:
            f[p:p + 2], f[p + 2:p + 4] = f[p + 2:p + 4], f[p:p + 2]
    if src is not None:
        f[a:a + w] = bytes(src)[:w].ljust(w, b"\0")
    if dst is not None:
        f[a + w:a + 2 * w] = bytes(dst)[:w].ljust(w, b"\0")
    if p is not None and sport is not None:
        f[p:p + 2] = int(sport).to_bytes(2, "big")
    if p is not None and dport is not None:
        f[p + 2:p + 4] = int(dport).to_bytes(2, "big")
    return repair(bytes(f))


_base = {}


def base(zp, golden):
    """Golden fixtures + generated c5 / c4 frames with their oracle records:
    (frames, recs). The keyed TCP / UDP ones without ip_in_ip are `ported`."""
    if not _base:
        frames = [bytes.fromhex(fx["bytes"]) for fx in golden["fixtures"]]
        for cfg, first in (("c5", 11), ("c4", 12)):
            arena, offs, lens = zp.batch.generate_host(cfg, 300, first=first)
            frames += [arena[o:o + l].tobytes() for o, l in zip(offs, lens)]
        recs, _ = orc.parse_batch(*pack(frames))
        fl = recs["flags"]
        ported = [i for i in range(len(frames)) if recs["err"][i] == 0 and fl[i] & (F_TCP | F_UDP)
                  and fl[i] & (ref.F_IPV4 | ref.F_IPV6) and not fl[i] & (1 << 4)]
        _base.update(frames=frames, recs=recs, ported=ported)
    return _base


def flow_frames(zp, golden, nflows, seed, reverse=0.0):
    """nflows frames with pairwise distinct (src address, src port), made from
    the ported base frames; a share `reverse` of them also with the endpoints
    swapped (the other direction of the same flow)."""
    b = base(zp, golden)
    rng = random.Random(seed)
    out = []
    for k in range(nflows):
        i = rng.choice(b["ported"])
        src = bytes([10 + k % 3, (k >> 8) & 0xFF, k & 0xFF, 7]) + bytes(rng.randrange(256) for _ in range(12))
        f = edit(b["frames"][i], b["recs"][i], src=src, sport=1024 + k, dport=rng.choice((53, 443, 8080)))
        out.append(f)
        if rng.random() < reverse:
            out.append(edit(f, b["recs"][i], swap=True))
    return out


def mixed_batch(zp, golden, n, nflows, seed, reverse=0.3):
    """About n frames: every golden fixture (rejected frames and ARP among
    them) and nflows flows (some in both directions) repeated, shuffled."""
    rng = random.Random(seed)
    flows = flow_frames(zp, golden, nflows, seed, reverse)
    frames = [bytes.fromhex(fx["bytes"]) for fx in golden["fixtures"]] + flows
    frames += [rng.choice(flows) for _ in range(max(0, n - len(frames)))]
    rng.shuffle(frames)
    return Batch(*pack(frames))


def describe(b, flags=FIVE, mask=None):
    """(keyed frames, F, flows with >= 2 frames) by the reference."""
    fo, ent, cnt = ref.aggregate(b.cols, b.packed, b.lens, opts_of(flags, b.n), mask)
    return cnt[1], cnt[0], int((ent["packets"] >= 2).sum())


def opts_of(flags, max_flows, hash_mask=None):
    import importlib
    return importlib.import_module("zero-packet_amd").flows.encode_opts(flags, max_flows, hash_mask)


# ---- CPU: the reference pinned by hand --------------------------------------

def golden_batch(golden):
    frames = [bytes.fromhex(fx["bytes"]) for fx in golden["fixtures"]]
    return Batch(*pack(frames))


def test_reference_on_the_golden_packets(zp, golden):
    b = golden_batch(golden)
    name = [fx["name"] for fx in golden["fixtures"]]
    assert name[1] == "vlan_tagged_frame" and name[15] == "arp_in_ethernet" and \
        name[13] == "ipv6_in_ipv4" and name[20] == "write_payload"
    not_keyed = [0, 15, 16, 17, 18]                       # the rejected fixtures (below 64 bytes)
    assert list(np.flatnonzero(~ref.keyed(b.packed))) == not_keyed
    assert all(b.recs["err"][i] != 0 for i in not_keyed)
    # an accepted frame without an IP reader is not keyed either: the ARP fixture padded to 64 bytes
    arp = Batch(*pack([bytes.fromhex(golden["fixtures"][15]["bytes"]) + bytes(22)]))
    assert arp.recs["err"][0] == 0 and arp.recs["flags"][0] == 0x3 and not ref.keyed(arp.packed).any()

    def groups(flags, mask=None):
        """The sets of fixtures that share a flow, and the reference's outputs."""
        fo, ent, cnt = ref.aggregate(b.cols, b.packed, b.lens, opts_of(flags, 100), mask)
        assert all(fo[i] == ref.NONE for i in not_keyed)
        g = {}
        for i, f in enumerate(fo):
            if f != ref.NONE:
                g.setdefault(int(f), []).append(i)
        assert list(ent["first"]) == [v[0] for v in g.values()] == sorted(ent["first"])
        assert list(ent["last"]) == [v[-1] for v in g.values()]
        assert list(ent["packets"]) == [len(v) for v in g.values()]
        assert cnt == [len(g), 19 - (0 if mask is None else int((~mask[ref.keyed(b.packed)]).sum())),
                       int(ent["bytes"].sum()), 0]
        return sorted(v for v in g.values() if len(v) > 1), ent, cnt
    # 1 and 2: 192.168.0.1:1234 -> 192.168.0.2:5678 UDP, VLAN 100 and 200
    shared, ent, cnt = groups(FIVE)
    assert shared == [[1, 2]] and cnt[0] == 18 and cnt[2] == int(b.lens.sum()) - 54 - 42 - 54 - 54 - 64
    assert ent["bytes"][0] == 128 and ent["tcp_flags"][0] == 0
    assert groups(FIVE | ref.VLAN)[0] == []
    # without the ports 7 and 8 (21004 / 21005 -> 135) merge; without the protocol 13 and 14
    # (ICMPv6 / ICMPv4 in 10.0.0.1 -> 10.0.0.2); 20 and 21 differ in ports only; 11, 19 and 22
    # are 2001:db8:: -> fe80:: with no L4, UDP and ICMPv6
    assert groups(ref.PROTO)[0] == [[1, 2], [7, 8], [20, 21]]
    assert groups(ref.PORTS)[0] == [[1, 2], [11, 22], [13, 14]]
    assert groups(0)[0] == [[1, 2], [7, 8], [11, 19, 22], [13, 14], [20, 21]]
    assert groups(ref.BIDIR)[0] == groups(0)[0]           # no fixture is another's reverse
    assert groups(ref.VLAN)[0] == [[7, 8], [11, 19], [13, 14]]     # 1 / 2, 20 / 21 and 22 by their tags
    # the key: under ip_in_ip the outer addresses (13: 10.0.0.1 -> 10.0.0.2, version 4) and the
    # innermost L4 (ICMPv6)
    _, ent, _ = groups(FIVE | ref.VLAN)
    k = ent["key"][12]
    assert ent["first"][12] == 13 and bytes(k["src_addr"]) == bytes([10, 0, 0, 1]) + bytes(12)
    assert bytes(k["dest_addr"]) == bytes([10, 0, 0, 2]) + bytes(12)
    assert (k["ip_version"], k["l4_proto"], k["src_port"], k["dest_port"], k["vlan"]) == (4, 58, 0, 0, 0)
    k = ent["key"][1]
    assert (k["src_port"], k["dest_port"], k["l4_proto"], k["vlan"]) == (1234, 5678, 17, 200)
    assert ent["tcp_flags"][5] == 0x12 and ent["first"][5] == 6       # the SYN-ACK of fixture 6
    # a mask leaves frames out: without 1, frame 2 is a flow of its own and comes first
    m = np.ones(b.n, bool)
    m[1] = False
    shared, ent, cnt = groups(FIVE, m)
    assert shared == [] and ent["first"][0] == 2 and cnt[0] == 18 and cnt[1] == 18


def test_reference_bidir_pair(zp, golden):
    """A -> B and B -> A, the second made by swapping the endpoints of the
    first: one flow under BIDIR, keyed by the smaller endpoint first."""
    b0 = golden_batch(golden)
    f = bytes.fromhex(golden["fixtures"][20]["bytes"])    # 192.168.1.1:12345 -> 192.168.1.2:54321
    back = edit(f, b0.recs[20], swap=True)
    same = edit(f, b0.recs[20], dst=bytes([192, 168, 1, 1]), dport=12345)    # equal endpoints
    hi = edit(f, b0.recs[20], dst=bytes([192, 168, 1, 1]), dport=12344)      # same address, port decides
    b = Batch(*pack([back, f, same, hi, edit(hi, b0.recs[20], swap=True)]))
    assert (b.recs["err"] == 0).all()
    assert bytes(b.cols["src_addr"][0][:4]) == bytes([192, 168, 1, 2]) and b.cols["src_port"][0] == 54321
    fo, ent, cnt = ref.aggregate(b.cols, b.packed, b.lens, opts_of(FIVE, 10))
    assert list(fo) == [0, 1, 2, 3, 4] and cnt[0] == 5
    fo, ent, cnt = ref.aggregate(b.cols, b.packed, b.lens, opts_of(FIVE | ref.BIDIR, 10))
    assert list(fo) == [0, 0, 1, 2, 2] and cnt == [3, 5, 320, 0]
    k = ent["key"][0]
    assert bytes(k["src_addr"][:4]) == bytes([192, 168, 1, 1]) and k["src_port"] == 12345 and \
        bytes(k["dest_addr"][:4]) == bytes([192, 168, 1, 2]) and k["dest_port"] == 54321
    assert (ent["first"][0], ent["last"][0], ent["packets"][0]) == (0, 1, 2)
    k = ent["key"][2]                                      # 192.168.1.1:12344 before 192.168.1.1:12345
    assert (k["src_port"], k["dest_port"]) == (12344, 12345)
    # without the ports the addresses alone decide: equal here, nothing swaps
    fo, _, _ = ref.aggregate(b.cols, b.packed, b.lens, opts_of(ref.PROTO | ref.BIDIR, 10))
    assert list(fo) == [0, 0, 1, 1, 1]


def test_layouts_and_constants(zp):
    fl = zp.flows
    assert fl.FLOW_DTYPE.itemsize == 64 and fl.KEY_DTYPE.itemsize == 40
    assert fl.FLOW_DTYPE == ref.FLOW_DTYPE and fl.KEY_DTYPE == ref.KEY_DTYPE
    assert [fl.FLOW_DTYPE.fields[k][1] for k in ("first", "last", "packets", "tcp_flags", "pad", "bytes")] \
        == [40, 44, 48, 52, 53, 56]
    assert [fl.KEY_DTYPE.fields[k][1] for k in ("src_addr", "dest_addr", "src_port", "dest_port",
                                                "l4_proto", "ip_version", "vlan")] == [0, 16, 32, 34, 36, 37, 38]
    o = fl.encode_opts(fl.PORTS | fl.BIDIR, 77, 5)
    assert o.tobytes() == (9).to_bytes(4, "little") + bytes(4) + (77).to_bytes(8, "little") + \
        (5).to_bytes(8, "little")
    assert fl.encode_opts(0, 1)[0]["hash_mask"] == 0xFFFFFFFFFFFFFFFF
    assert fl.key_flags() == FIVE and fl.key_flags(False, False, True, True) == fl.VLAN | fl.BIDIR
    hdr = open(os.path.join(ROOT, "include", "zero_packet.h")).read()
    for name, v in (("PORTS", fl.PORTS), ("PROTO", fl.PROTO), ("VLAN", fl.VLAN), ("BIDIR", fl.BIDIR)):
        assert int(re.search(rf"#define ZP_FLOW_{name}\s+(\d+)u", hdr).group(1)) == v == getattr(ref, name)
    assert int(re.search(r"#define ZP_FLOW_NONE\s+0x([0-9A-F]+)u", hdr).group(1), 16) == fl.FLOW_NONE == ref.NONE
    assert int(re.search(r"#define ZP_ABI_VERSION (\d+)", hdr).group(1)) == 6 == zp._lib.hip().zp_abi_version()
    for bad in (lambda: fl.encode_opts(16, 1), lambda: fl.encode_opts(0, 0), lambda: fl.encode_opts(0, -1),
                lambda: fl.encode_opts(0, 1, 1 << 64)):
        with pytest.raises(ValueError):
            bad()


def test_scratch_bound(zp):
    """zp_flow_scratch_bytes is at most 64 B per frame + 64 B per max_flows +
    a constant (4,096 B), and grows with both."""
    lib = zp._lib.hip()
    sb = lambda n, m: int(lib.zp_flow_scratch_bytes(n, m))
    for n in (0, 1, 63, 64, 65, 1000, 4096, 262144, 262145, (1 << 24) + 5, 1 << 28):
        for m in (1, 2, 31, 32, 33, 1000, 4096, 1 << 20, (1 << 30) + 3, 1 << 40, (1 << 64) - 1):
            assert 0 < sb(n, m) <= 64 * n + 64 * m + 4096, (n, m)
            assert sb(n, m) >= 48 * n + 8 * 2 * min(n, m)         # the rows and a half-empty table
    assert sb(1000, 10) < sb(1000, 1000) == sb(1000, 1 << 40)      # more than n flows cannot occur
    assert sb(1000, 1000) < sb(2000, 1000)


def test_refusals_touch_no_device(zp):
    """Every refusal returns negative with its cause named, before any HIP
    call: the pointers given are never dereferenced."""
    lib, fl = zp._lib.hip(), zp.flows
    P = 4096                                              # a non-null "device pointer"
    big = int(lib.zp_flow_scratch_bytes(1000, 100))

    def call(enc, arena=P, offs=P, lens=P, recs=P, n=1000, mask=None, flow_of=P, flows=P, count=P,
             scratch=P, nscratch=big):
        return lib.zp_flow_aggregate_device(arena, offs, lens, recs, n,
                                            enc.ctypes.data if enc is not None else None, mask,
                                            flow_of, flows, count, scratch, nscratch, None)

    def refused(what, *a, **kw):
        assert call(*a, **kw) < 0, what
        msg = lib.zp_last_error().decode()
        assert msg.startswith("zp_flow_aggregate_device: ") and what in msg, (what, msg)
    ok = fl.encode_opts(FIVE, 100)
    refused("null opts", None)
    refused("null records", ok, recs=None)
    refused("null lens", ok, lens=None)
    refused("null arena", ok, arena=None)
    refused("null offs", ok, offs=None)
    refused("null flows", ok, flows=None)
    refused("null count", ok, count=None)
    refused("scratch", ok, scratch=None)
    refused("scratch", ok, nscratch=big - 1)
    e = ok.copy(); e["key_flags"] = 16
    refused("unknown key_flags", e)
    e = ok.copy(); e["key_flags"] = 0x80000001
    refused("unknown key_flags", e)
    e = ok.copy(); e["pad"] = 1
    refused("pad", e)
    e = ok.copy(); e["max_flows"] = 0
    refused("max_flows", e)
    refused("2^32", ok, n=1 << 32, nscratch=1 << 62)
    refused("misaligned", ok, flows=P + 4)
    refused("misaligned", ok, flow_of=P + 2)
    refused("misaligned", ok, count=P + 4)
    refused("misaligned", ok, mask=P + 1)


def test_facade_argument_checks(zp):
    import torch
    fl = zp.flows
    a = torch.zeros(128, dtype=torch.uint8)
    o = torch.zeros(1, dtype=torch.int64)
    l_ = torch.full((1,), 64, dtype=torch.int32)
    r = torch.zeros((1, 8), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="device tensors"):
        fl.aggregate(a, o, l_, r)
    with pytest.raises(ValueError, match="unknown outputs"):
        fl.aggregate(a, o, l_, r, want=("flow_of", "idx"))
    assert fl.aggregate.__defaults__[:4] == (True, True, False, False)
    assert "SYNCHRONISATION" in fl.to_numpy.__doc__


# ---- GPU --------------------------------------------------------------------

def run(zp, b, flags=FIVE, max_flows=None, mask=None, hash_mask=None, scratch_fill=None, **kw):
    """aggregate() into guard-filled outputs -> (count list, entries bytes of
    the first F, flow_of uint32 array, the raw output tensors)."""
    import torch
    fl = zp.flows
    da, do, dl, dr = b.device()
    cap = b.n if max_flows is None else max_flows
    out = {"count": torch.full((4,), -1, dtype=torch.int64, device=dev()),
           "flows": torch.full((cap + 2, 64), GUARD, dtype=torch.uint8, device=dev()),
           "flow_of": torch.full((b.n + 8,), -1431655766, dtype=torch.int32, device=dev())}
    if scratch_fill is not None:
        nb = int(zp._lib.hip().zp_flow_scratch_bytes(b.n, cap))
        out["scratch"] = torch.full((nb,), scratch_fill, dtype=torch.uint8, device=dev())
    t = fl.aggregate(da, do, dl, dr, ports=bool(flags & ref.PORTS), proto=bool(flags & ref.PROTO),
                     vlan=bool(flags & ref.VLAN), bidir=bool(flags & ref.BIDIR), max_flows=cap,
                     mask=mask, out=out, hash_mask=hash_mask, **kw)
    return t


def read(t, n, cap):
    count = [int(v) for v in t.count.tolist()]
    flows = t.flows.cpu().numpy()
    fo = t.flow_of.cpu().numpy().view(np.uint32)
    assert (fo[n:] == 0xAAAAAAAA).all(), "flow_of written past n"
    assert (flows[cap:] == GUARD).all(), "flows written past max_flows"
    return count, flows, fo[:n]


def check_flows(zp, b, flags=FIVE, max_flows=None, mask=None, want=None, **kw):
    """Runs on the device and compares everything with flow_ref; returns the
    reference's (flow_of, entries, count) and the device result's bytes."""
    cap = b.n if max_flows is None else max_flows
    dmask = None
    if mask is not None:
        dmask, = to_dev(select_ref.mask_words(mask))
    t = run(zp, b, flags, max_flows, dmask, **kw)
    count, flows, fo = read(t, b.n, cap)
    wfo, went, wcnt = want or ref.aggregate(b.cols, b.packed, b.lens, opts_of(flags, cap), mask)
    assert count == wcnt, (count, wcnt)
    assert wcnt[3] == 0
    f = wcnt[0]
    assert np.array_equal(fo, wfo), np.flatnonzero(fo != wfo)[:8]
    got = flows[:f].reshape(-1).view(ref.FLOW_DTYPE)
    assert got.tobytes() == went.tobytes(), [
        (i, got[i], went[i]) for i in range(f) if got[i].tobytes() != went[i].tobytes()][:2]
    assert (flows[f:] == GUARD).all(), "entries at and past F were written"
    assert zp.flows.to_numpy(t).tobytes() == went.tobytes()
    return (wfo, went, wcnt), (count, flows[:f].tobytes(), fo.tobytes())


_mixed = {}


def mixed(zp, golden):
    if "b" not in _mixed:
        _mixed["b"] = mixed_batch(zp, golden, 2000, 150, seed=5)
    return _mixed["b"]


def test_mixed_batch_properties(zp, golden):
    """CPU: the batch most GPU tests share has flows of several frames, frames
    that are not keyed, and pairs only BIDIR merges."""
    b = mixed(zp, golden)
    keyed, f, multi = describe(b)
    assert 1900 <= b.n <= 2100 and keyed < b.n and (b.recs["err"] != 0).sum() >= 4
    assert f >= 150 and multi >= 100
    assert describe(b, FIVE | ref.BIDIR)[1] <= f - 20      # directions merged
    assert describe(b, FIVE | ref.VLAN)[1] > f             # the golden VLAN pair split
    assert describe(b, ref.PROTO)[1] < f
    assert len({describe(b, k)[1] for k in range(16)}) >= 6


@pytest.mark.gpu
@pytest.mark.parametrize("flags", range(16))
def test_key_flags(zp, golden, flags):
    check_flows(zp, mixed(zp, golden), flags)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_batch_sizes(zp, golden, n):
    b0 = mixed(zp, golden)
    # from frame 3 on: the first frame of the batch is keyed for n == 1
    start = int(np.flatnonzero(ref.keyed(b0.packed))[0])
    b = Batch(b0.arena, b0.offs[start:start + n], b0.lens[start:start + n])
    keyed, f, multi = describe(b)
    assert b.n == n and keyed >= 1 and (n < 63 or multi >= 2) and (n < 1000 or keyed < n)
    check_flows(zp, b)
    check_flows(zp, b, FIVE | ref.BIDIR | ref.VLAN)


@pytest.mark.gpu
def test_one_flow(zp, golden):
    f = flow_frames(zp, golden, 1, seed=3)[0]
    b = Batch(*pack([f] * 4096))
    (_, ent, cnt), _ = check_flows(zp, b)
    assert cnt[:2] == [1, 4096] and cnt[2] == 4096 * len(f)
    assert (ent["packets"][0], ent["first"][0], ent["last"][0]) == (4096, 0, 4095)
    lib = zp._lib.hip()
    was = lib.zp__flow_combine(0)                          # and without the in-wave combining
    try:
        check_flows(zp, b)
    finally:
        lib.zp__flow_combine(was)


@pytest.mark.gpu
def test_all_distinct(zp, golden):
    frames = flow_frames(zp, golden, 4096, seed=4)
    b = Batch(*pack(frames))
    assert len(set(zip(b.cols["src_port"].tolist(), b.cols["dest_port"].tolist()))) == 4096
    (_, ent, cnt), _ = check_flows(zp, b)
    assert cnt[0] == 4096 and (ent["packets"] == 1).all() and (ent["first"] == np.arange(4096)).all()
    lib = zp._lib.hip()
    was = lib.zp__flow_combine(0)
    try:
        check_flows(zp, b)
    finally:
        lib.zp__flow_combine(was)


@pytest.mark.gpu
@pytest.mark.parametrize("hash_mask", [0, 1, 7])
def test_forced_collisions(zp, golden, hash_mask):
    """Every key on one, two or eight probe chains: the probe walks past
    foreign keys and only the comparison of the whole key tells flows apart."""
    b = mixed(zp, golden)
    assert describe(b)[1] >= 150
    want, full = check_flows(zp, b, hash_mask=0xFFFFFFFFFFFFFFFF)
    _, got = check_flows(zp, b, hash_mask=hash_mask, want=want)
    assert got == full
    _, got = check_flows(zp, b, FIVE | ref.BIDIR, hash_mask=hash_mask)
    assert got == check_flows(zp, b, FIVE | ref.BIDIR)[1]


@pytest.mark.gpu
def test_bidir(zp, golden):
    bs = base(zp, golden)
    g = golden["fixtures"]
    f = bytes.fromhex(g[20]["bytes"])                      # IPv4 UDP 192.168.1.1:12345 -> .2:54321
    r20 = bs["recs"][20]
    f6 = bytes.fromhex(g[5]["bytes"])                      # IPv6 UDP
    r5 = bs["recs"][5]
    assert g[5]["name"] == "ipv6_udp_payload" and g[20]["name"] == "write_payload"
    v4 = edit(f, r20, src=bytes([10, 0, 0, 1]), dst=bytes([10, 0, 0, 2]), sport=7, dport=9)
    v6 = edit(f6, r5, src=bytes([10, 0, 0, 1]) + bytes(12), dst=bytes([10, 0, 0, 2]) + bytes(12),
              sport=7, dport=9)
    frames = [edit(f, r20, swap=True), f,                                    # B -> A, A -> B
              edit(f, r20, dst=bytes([192, 168, 1, 1]), dport=12345),        # equal endpoints
              edit(f, r20, dst=bytes([192, 168, 1, 1]), dport=12344),        # the port decides
              edit(f, r20, src=bytes([192, 168, 1, 1]), sport=12344, dst=bytes([192, 168, 1, 1]), dport=12345),
              v4, v6, edit(v4, r20, swap=True), edit(v6, r5, swap=True)]
    frames = frames * 40 + flow_frames(zp, golden, 60, seed=8, reverse=0.5)
    random.Random(2).shuffle(frames)
    b = Batch(*pack(frames))
    assert (b.recs["err"] == 0).all()
    same4 = np.flatnonzero((b.cols["ip_version"] == 4) & (b.cols["src_addr"][:, :4] == [10, 0, 0, 1]).all(1)
                           & (b.cols["src_port"] == 7))
    same6 = np.flatnonzero((b.cols["ip_version"] == 6) & (b.cols["src_addr"][:, :4] == [10, 0, 0, 1]).all(1)
                           & (b.cols["src_addr"][:, 4:] == 0).all(1))
    assert len(same4) == 40 and len(same6) == 40
    for flags in (FIVE | ref.BIDIR, ref.PROTO | ref.BIDIR, ref.BIDIR, FIVE):
        (fo, ent, cnt), _ = check_flows(zp, b, flags)
        assert fo[same4[0]] != fo[same6[0]], "an IPv4 and an IPv6 flow with the same leading bytes"
        if flags & ref.BIDIR:
            assert cnt[0] < describe(b, flags & ~ref.BIDIR)[1] - 20


@pytest.mark.gpu
def test_no_keyed_frames(zp, golden):
    g = [bytes.fromhex(fx["bytes"]) for fx in golden["fixtures"]]
    frames = [g[i] for i in (0, 16, 17, 18)] * 120 + [g[15] + bytes(22)] * 120    # ARP, padded to 64 B
    random.Random(6).shuffle(frames)
    b = Batch(*pack(frames))
    assert not ref.keyed(b.packed).any() and (b.recs["err"] == 0).sum() == 120     # the ARP frames
    (fo, ent, cnt), _ = check_flows(zp, b)
    assert cnt == [0, 0, 0, 0] and (fo == ref.NONE).all()


@pytest.mark.gpu
def test_mask_from_select(zp, golden):
    b = mixed(zp, golden)
    da, do, dl, dr = b.device()
    sel = zp.select.Select(ok=True).where("l4_proto", eq=17)
    s = zp.select.run(da, do, dl, dr, sel, want=("mask",))
    m = select_ref.select_mask(sel.encode(), b.cols, b.packed, b.lens)
    assert 100 < m.sum() < ref.keyed(b.packed).sum()
    t = run(zp, b, mask=s.mask)
    count, flows, fo = read(t, b.n, b.n)
    wfo, went, wcnt = ref.aggregate(b.cols, b.packed, b.lens, opts_of(FIVE, b.n), m)
    assert count == wcnt and np.array_equal(fo, wfo)
    assert flows[:wcnt[0]].tobytes() == went.tobytes()
    assert (went["key"]["l4_proto"] == 17).all() and wcnt[0] < describe(b)[1]
    check_flows(zp, b, FIVE | ref.BIDIR, mask=m)


@pytest.mark.gpu
def test_overflow(zp, golden):
    b = mixed(zp, golden)
    f = describe(b)[1]
    assert f >= 150
    check_flows(zp, b, max_flows=f)                        # exactly full: exact, no overflow
    for cap in (f - 1, 1, 40):
        t = run(zp, b, max_flows=cap)
        count, flows, fo = read(t, b.n, cap)               # the guards behind flows and flow_of
        assert count[3] == 1, cap
    t = run(zp, b, max_flows=f + 1000)
    assert read(t, b.n, f + 1000)[0][3] == 0


@pytest.mark.gpu
def test_scan_boundary(zp):
    """One frame past a scan workgroup's span, and heads in the last tile:
    the rank scan's second level runs."""
    import torch
    n = zp.select.SCAN_FRAMES + 300
    da, do, dl = zp.batch.generate("c2", n, first=77, device=dev())
    dr, _ = zp.batch.parse_batch(da, do, dl)
    torch.cuda.synchronize()
    b = Batch(da.cpu().numpy(), do.cpu().numpy(), dl.cpu().numpy())
    b.d = [da, do, dl, dr]
    assert dr.cpu().numpy().tobytes() == b.packed.tobytes()
    want = ref.aggregate(b.cols, b.packed, b.lens, opts_of(FIVE, n))
    assert want[2][0] > 1000 and want[1]["first"].max() >= zp.select.SCAN_FRAMES, \
        "flows that begin past the first scan span"
    check_flows(zp, b, want=want)


@pytest.mark.gpu
def test_layouts(zp, golden):
    """Frames at odd offsets with gaps (test_columns.pack), the descriptors
    shuffled, and frames whose L4 header lies far into the frame."""
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
    k = len(frames) - 3
    assert (b.recs["l4_off"] > 0x3FFFF).any() and describe(b)[2] >= 50
    (fo, ent, _), _ = check_flows(zp, b)
    where = {int(v): j for j, v in enumerate(p)}
    for j in range(3):                                     # each far frame twice: one flow of two
        assert fo[where[300 + j]] == fo[where[k + j]] != ref.NONE
    check_flows(zp, b, FIVE | ref.BIDIR | ref.VLAN)


@pytest.mark.gpu
def test_dirty_scratch_and_determinism(zp, golden):
    b = mixed(zp, golden)
    _, first = check_flows(zp, b)
    _, again = check_flows(zp, b)
    assert first == again
    for fill in (0xFF, 0x00, 0x5A):
        _, got = check_flows(zp, b, scratch_fill=fill)
        assert got == first, fill


@pytest.mark.gpu
def test_graph_replay(zp, golden):
    """aggregate(check=False) captured and replayed twice: the same bytes as
    the eager call."""
    import torch
    b = mixed(zp, golden)
    _, eager = check_flows(zp, b, FIVE | ref.BIDIR)
    da, do, dl, dr = b.device()
    out = {"count": torch.zeros(4, dtype=torch.int64, device=dev()),
           "flows": torch.zeros((b.n, 64), dtype=torch.uint8, device=dev()),
           "flow_of": torch.zeros(b.n, dtype=torch.int32, device=dev()),
           "scratch": torch.zeros(int(zp._lib.hip().zp_flow_scratch_bytes(b.n, b.n)), dtype=torch.uint8,
                                  device=dev())}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                          # warm up outside the capture
        zp.flows.aggregate(da, do, dl, dr, bidir=True, out=out, check=False)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        t = zp.flows.aggregate(da, do, dl, dr, bidir=True, out=out, check=False)
    for _ in range(2):
        for v in out.values():
            v.fill_(0x33)
        g.replay()
        torch.cuda.synchronize()
        count = [int(v) for v in t.count.tolist()]
        got = (count, t.flows.cpu().numpy()[:count[0]].tobytes(),
               t.flow_of.cpu().numpy().view(np.uint32).tobytes())
        assert got == eager
