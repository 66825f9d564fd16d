"""Route (zp_route_compile, zp_route_lookup_host, zp_route_device, routes.py).

CPU: tests/route_ref.py pinned on the golden packets by hand-written
expectations and against the standard library's ipaddress; the compiled
table through zp_route_lookup_host (every length of interest, first / last /
neighbouring addresses, nested chains, the IPv4 / IPv6 aliasing pair), its
determinism and size bound, every refusal of compile and of zp_route_device
(they return before any HIP call), a corrupted body, and the stand-alone
sanitizer program.
GPU: value_of and the mask words equal route_ref as whole arrays, in
sentinel-filled buffers 64 entries longer than the batch.
"""
import ctypes
import ipaddress
import mmap
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import oracle as orc
import route_ref as rref
import select_ref as sref
from test_columns import pack
from test_select import Batch, corpus, dev, golden_batch, to_dev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [c[0] for c in orc.COLUMN_SPEC]
NONE = rref.NONE
LENS = {4: [0, 1, 15, 16, 17, 23, 24, 25, 31, 32],
        6: [0, 1, 16, 17, 24, 63, 64, 65, 120, 121, 127, 128]}
WIDTH = {4: 32, 6: 128}
HDR_BYTES, ROOT_BYTES, NODE_BYTES = 64, 512 << 10, 1 << 10


def trunc(addr, length):
    """The 16 address bytes with everything past `length` bits cleared."""
    return bytes(np.frombuffer(bytes(addr), np.uint8) & rref.len_mask(length))


def raw_prefixes(zp, items):
    """PREFIX_DTYPE from (version, len, 16 address bytes, value) tuples."""
    enc = np.zeros(len(items), zp.routes.PREFIX_DTYPE)
    for k, (version, length, addr, value) in enumerate(items):
        enc[k]["addr"] = np.frombuffer(bytes(addr), np.uint8)
        enc[k]["len"], enc[k]["version"], enc[k]["value"] = length, version, value
    return enc


def chains(zp, addrs, caps=None, first_value=100):
    """For every (version, 16 bytes) of addrs the address truncated to each
    length of interest (up to caps[k], when given): nested chains, one
    distinct value per prefix."""
    seen, items = set(), []
    for k, (version, addr) in enumerate(addrs):
        for length in LENS[version]:
            if caps is not None and length > caps[k]:
                continue
            key = (version, length, trunc(addr, length))
            if key not in seen:
                seen.add(key)
                items.append(key + (first_value + len(items),))
    return raw_prefixes(zp, items)


def ip(text):
    a = ipaddress.ip_address(text)
    return a.version, a.packed + bytes(16 - len(a.packed))


def bound(enc):
    """The size bound include/zero_packet.h states."""
    lv = np.maximum(0, (enc["len"].astype(np.int64) - 16 + 7) // 8)
    return HDR_BYTES + ROOT_BYTES + NODE_BYTES * int(lv.sum())


# ---- CPU: the reference pinned ----------------------------------------------

GOLDEN_TABLE = [("192.168.0.0/16", 1), ("192.168.1.0/24", 2), ("192.168.1.2/32", 3),
                ("10.0.0.0/8", 4), ("0.0.0.0/0", 5), ("fe80::/10", 10),
                ("fe80::202:b3ff:fe1e:8329/128", 11), ("fc00:2::/32", 12),
                ("fc00:2:0:5::/64", 13), ("2::/16", 14), ("a00::/8", 15)]


def test_reference_on_the_golden_packets(zp, golden):
    arena, offs, lens, recs, ext, cols, packed = golden_batch(golden)
    name = [fx["name"] for fx in golden["fixtures"]]
    assert name[13] == "ipv6_in_ipv4" and name[12] == "ipv6_in_ipv6_with_extension_header"
    enc = zp.routes.encode_prefixes(GOLDEN_TABLE)
    N = NONE
    # dest: 192.168.0.2 x2, 139.133.217.110 (default), fe80::260.., 3ffe:501.. (no IPv6 default),
    # fc00:2:0:2::1, 2::1 x2, 2001:41d0.., fe80::21e.., fe80::202:b3ff:fe1e:8329, fc00:2:0:5::1,
    # 10.0.0.2 x2 (the outer header; never the IPv6 prefix a00::/8), four error frames, ...
    want_dest = [N, 1, 1, 5, 10, N, 12, 14, 14, N, 10, 11, 13, 4, 4, N, N, N, N, 11, 3, 3, 11, N]
    want_src = [N, 1, 1, 5, 10, N, 12, 14, 14, N, 10, N, N, 4, 4, N, N, N, N, N, 2, 2, N, N]
    got, prefix = rref.match(enc, cols, packed, "dest_addr")
    assert got.tolist() == want_dest
    assert rref.value_of(enc, cols, packed, "src_addr").tolist() == want_src
    assert rref.depth(enc, prefix)[[1, 3, 20, 12, 11, 0]].tolist() == [1, 1, 3, 7, 15, 0]
    assert rref.mask_words(got)[0] == sum(1 << i for i, v in enumerate(want_dest) if v != N)
    # only: a clear bit is not routed
    only = np.zeros(24, bool)
    only[[1, 4, 15]] = True
    got = rref.value_of(enc, cols, packed, "dest_addr", only)
    assert got[1] == 1 and got[4] == 10 and (np.delete(got, [1, 4]) == N).all()
    # without the IPv4 default: 139.133.217.110 falls to NONE; an IPv6 default takes the rest
    enc2 = zp.routes.encode_prefixes([p for p in GOLDEN_TABLE if p[1] != 5] + [("::/0", 6)])
    got = rref.value_of(enc2, cols, packed, "dest_addr")
    assert got[3] == N and got[[5, 9, 23]].tolist() == [6, 6, 6] and got[13] == 4


def test_reference_against_ipaddress():
    """route_ref.match_addrs against `addr in network` of the standard
    library on a few thousand random (address, table) pairs."""
    rng = np.random.default_rng(11)
    dt = np.dtype([("addr", "u1", (16,)), ("len", "u1"), ("version", "u1"), ("pad", "u1", (2,)),
                   ("value", "<u4")])
    pairs = 0
    for t in range(60):
        version = 4 if t % 2 == 0 else 6
        nb = 4 if version == 4 else 16
        base = rng.integers(0, 256, (6, 16)).astype(np.uint8)
        base[:, nb:] = 0
        nets, seen = [], set()
        for k in range(40):
            length = int(rng.choice(LENS[version] + [8, 20, 28]))
            a = trunc(base[rng.integers(0, 6)], length)
            if (length, a) not in seen:
                seen.add((length, a))
                nets.append((ipaddress.ip_network((a[:nb], length)), length, a, 7 + k))
        enc = np.zeros(len(nets), dt)
        for k, (_, length, a, value) in enumerate(nets):
            enc[k] = (np.frombuffer(a, np.uint8), length, version, [0, 0], value)
        # addresses near the bases (they share long prefixes with the networks) and random ones
        addrs = np.concatenate([base.repeat(8, 0), rng.integers(0, 256, (12, 16)).astype(np.uint8)])
        addrs[:48, nb - 1] ^= rng.integers(0, 4, 48).astype(np.uint8)
        addrs[:, nb:] = 0
        got, _ = rref.match_addrs(enc, addrs, np.full(len(addrs), version))
        other, _ = rref.match_addrs(enc, addrs, np.full(len(addrs), 10 - version))
        assert (other == NONE).all(), "the version is part of the match"
        for a, g in zip(addrs, got):
            ia = ipaddress.ip_address(bytes(a[:nb]))
            best = max((n for n in nets if ia in n[0]), key=lambda n: n[1], default=None)
            assert int(g) == (best[3] if best else NONE)
            pairs += 1
    assert pairs >= 3000


# ---- CPU: the compiled table through zp_route_lookup_host -------------------

def lookup_all(zp, table, addrs):
    """zp_route_lookup_host for (version, 16 bytes) pairs -> uint32 array."""
    return np.array([zp.routes.lookup_host(table, (a, v)) for v, a in addrs], np.uint32)


def ref_all(enc, addrs):
    a = np.array([np.frombuffer(x, np.uint8) for _, x in addrs]).reshape(len(addrs), 16)
    return rref.match_addrs(enc, a, np.array([v for v, _ in addrs]))[0]


def edge_addresses(enc):
    """Per prefix: its first and last address and the neighbours just outside."""
    out = []
    for p in enc:
        version, length = int(p["version"]), int(p["len"])
        w = WIDTH[version]
        lo = int.from_bytes(bytes(p["addr"][:w // 8]), "big")
        hi = lo | ((1 << (w - length)) - 1)
        for x in (lo, hi, lo - 1, hi + 1):
            if 0 <= x < 1 << w:
                out.append((version, x.to_bytes(w // 8, "big") + bytes(16 - w // 8)))
    return out


def every_length_tables(zp):
    """Tables that hold every length of interest: nested chains over a few
    addresses of both versions (with and without the defaults), and the
    IPv4 / IPv6 aliasing pair."""
    rng = np.random.default_rng(5)
    seeds = [ip("10.0.0.1"), ip("10.0.0.2"), ip("10.1.255.255"), ip("255.255.255.255"), ip("0.0.0.0"),
             ip("a00:1::"), ip("a00:1::1"), ip("2001:db8:85a3::8a2e:370:7334"), ip("::"),
             ip("ffff:ffff:ffff:ffff:ffff:ffff:ffff:ffff")]
    for _ in range(6):
        seeds.append((4, bytes(rng.integers(0, 256, 4).astype(np.uint8)) + bytes(12)))
        seeds.append((6, bytes(rng.integers(0, 256, 16).astype(np.uint8))))
    full = chains(zp, seeds)
    yield "chains", full, seeds
    yield "no defaults", full[full["len"] > 1], seeds
    yield "v4 only", full[full["version"] == 4], seeds
    alias = zp.routes.encode_prefixes([("a00:1::/32", 66), ("10.0.0.0/8", 44)])
    yield "aliasing", alias, [ip("10.0.0.1"), ip("a00:1::1"), ip("a00:1::")]
    yield "empty", full[:0], seeds
    yield "defaults", zp.routes.encode_prefixes([("0.0.0.0/0", 1)]), seeds


def test_host_lookup_equals_reference(zp):
    R = zp.routes
    for name, enc, seeds in every_length_tables(zp):
        table = R.compile_prefixes(enc)
        addrs = edge_addresses(enc) + list(seeds)
        # every address under the other version too: nothing may alias
        addrs += [(10 - v, a[:4] + bytes(12) if v == 6 else a) for v, a in addrs[:200]]
        got, want = lookup_all(zp, table, addrs), ref_all(enc, addrs)
        assert np.array_equal(got, want), (name, np.flatnonzero(got != want)[:8])
        if name == "chains":
            for version in (4, 6):
                assert set(enc["len"][enc["version"] == version].tolist()) == set(LENS[version])
            # a chain's own address is covered by prefixes of every length: the longest answers
            own = ref_all(enc, seeds)
            assert len(set(own.tolist())) == len(seeds)
            assert (want == NONE).sum() == 0 and len(set(want.tolist())) > 100
        elif name == "no defaults":
            assert (want == NONE).any() and (want != NONE).any()
        elif name == "aliasing":
            assert lookup_all(zp, table, seeds).tolist() == [44, 66, 66]
            # the same bytes under the other version: the version picks the root
            assert R.lookup_host(table, (ip("10.0.0.1")[1], 6)) == 66
            assert R.lookup_host(table, (ip("a00:1::")[1], 4)) == 44
        elif name == "empty":
            assert (got == NONE).all() and table.size == HDR_BYTES + ROOT_BYTES
        elif name == "defaults":
            assert set(got[[v == 4 for v, _ in addrs]].tolist()) == {1}
            assert set(got[[v == 6 for v, _ in addrs]].tolist()) == {NONE}
        # a version that is neither is NONE
        assert R.lookup_host(table, (seeds[0][1], 5)) == NONE


def test_facade_encode_and_lookup(zp):
    R = zp.routes
    enc = R.encode_prefixes({"10.0.0.0/8": 1, ipaddress.ip_network("2001:db8::/32"): 2})
    assert enc.dtype == R.PREFIX_DTYPE and enc.itemsize == 24
    assert bytes(enc[0]["addr"]) == bytes([10]) + bytes(15) and (enc[0]["len"], enc[0]["version"]) == (8, 4)
    assert bytes(enc[1]["addr"]) == bytes.fromhex("20010db8") + bytes(12) and enc[1]["value"] == 2
    with pytest.raises(ValueError):
        R.encode_prefixes([("10.1.2.3/8", 1)])
    loose = R.encode_prefixes([("10.1.2.3/8", 1)], strict=False)
    assert bytes(loose[0]["addr"]) == bytes([10]) + bytes(15)
    with pytest.raises(ValueError):
        R.encode_prefixes([("10.0.0.0/8", R.VALUE_MAX + 1)])
    table = R.compile_prefixes(enc)
    assert R.lookup_host(table, "10.9.9.9") == 1 and R.lookup_host(table, "11.0.0.0") == NONE
    assert R.lookup_host(table, ipaddress.ip_address("2001:db8::1")) == 2
    with pytest.raises(RuntimeError):
        R.RouteTable(enc, "cpu")


def test_constants(zp):
    R = zp.routes
    hdr = open(os.path.join(ROOT, "include", "zero_packet.h")).read()
    assert int(re.search(r"#define ZP_ROUTE_NONE\s+(0x[0-9A-Fa-f]+)u", hdr).group(1), 16) == R.ROUTE_NONE
    assert int(re.search(r"#define ZP_ROUTE_VALUE_MAX\s+(0x[0-9A-Fa-f]+)u", hdr).group(1), 16) == R.VALUE_MAX
    assert re.search(r"#define ZP_ROUTE_MAX_PREFIXES\s+\(1u << 20\)", hdr) and R.MAX_PREFIXES == 1 << 20
    assert re.search(r"#define ZP_ABI_VERSION 6\b", hdr)
    assert R.PREFIX_DTYPE.itemsize == 24 and R.PREFIX_DTYPE.fields["value"][1] == 20
    assert R.ROUTE_NONE == NONE == zp.classify.RULE_NONE
    assert NAMES.index("dest_addr") == zp.columns.INDEX["dest_addr"]


# ---- CPU: compile -----------------------------------------------------------

def test_compile_is_deterministic_and_sized(zp):
    lib = zp._lib.hip()
    rng = np.random.default_rng(3)
    for name, enc, _ in every_length_tables(zp):
        nb = int(lib.zp_route_table_bytes(enc.ctypes.data, len(enc)))
        assert HDR_BYTES + ROOT_BYTES <= nb <= bound(enc) and (nb - HDR_BYTES) % NODE_BYTES == 0, name
        outs = []
        for k in range(5):
            perm = enc[rng.permutation(len(enc))] if k else enc
            for fill in (0x00, 0xA5):
                t = np.full(nb // 8 + 8, fill * 0x0101010101010101, np.uint64)
                assert lib.zp_route_table_bytes(perm.ctypes.data, len(perm)) == nb
                assert lib.zp_route_compile(perm.ctypes.data, len(perm), t.ctypes.data, nb + 64) == 0
                assert (t[nb // 8:] == fill * 0x0101010101010101).all(), "written past table_bytes"
                outs.append(t[:nb // 8].tobytes())
        assert all(o == outs[0] for o in outs), name
        assert zp.routes.compile_prefixes(enc).tobytes() == outs[0]
        w = np.frombuffer(outs[0], "<u4")
        assert w[2] == len(enc) and w[4] == nb and w[5] == 0 and not w[6:16].any()
        assert nb == HDR_BYTES + ROOT_BYTES + NODE_BYTES * int(w[3])
    # other values, other bytes; disjoint /32s meet the bound exactly
    enc = chains(zp, [ip("10.0.0.1")])
    other = enc.copy()
    other[3]["value"] += 1
    assert zp.routes.compile_prefixes(other).tobytes() != zp.routes.compile_prefixes(enc).tobytes()
    apart = raw_prefixes(zp, [(4, 32, bytes([k, k, k, k]) + bytes(12), k) for k in range(9)])
    assert lib.zp_route_table_bytes(apart.ctypes.data, 9) == bound(apart) == \
        HDR_BYTES + ROOT_BYTES + 18 * NODE_BYTES


def test_compile_refusals(zp):
    R, lib = zp.routes, zp._lib.hip()
    good = R.encode_prefixes([("10.0.0.0/8", 1), ("10.1.0.0/16", 2), ("2001:db8::/32", 3),
                              ("10.1.2.0/24", 4), ("10.1.2.3/32", 5)])
    nb = int(lib.zp_route_table_bytes(good.ctypes.data, 5))
    # nodes: 10.1 and 10.1.2 (the /24 and the /32 share the first), 2001 and 2001:0d
    assert nb == HDR_BYTES + ROOT_BYTES + 4 * NODE_BYTES
    buf = np.full(nb // 8, 0x5A5A5A5A5A5A5A5A, np.uint64)

    def refused(what, enc, n=5, nbytes=nb, table=buf, sized=True):
        p = enc.ctypes.data if enc is not None else None
        rc = lib.zp_route_compile(p, n, table.ctypes.data if table is not None else None, nbytes)
        assert rc < 0, what
        msg = lib.zp_last_error().decode()
        assert "zp_route_compile" in msg and what in msg, (what, msg)
        assert (buf == 0x5A5A5A5A5A5A5A5A).all(), "the table was touched by a refused compile"
        if sized:                                         # and zp_route_table_bytes says 0 for it
            assert lib.zp_route_table_bytes(p, n) == 0
            assert "zp_route_table_bytes" in lib.zp_last_error().decode()
    for i in (0, 2, 4):
        e = good.copy(); e[i]["version"] = 5
        refused(f"prefix {i}: version 5", e)
        e = good.copy(); e[i]["len"] = 129 if e[i]["version"] == 6 else 33
        refused(f"prefix {i}: len", e)
        e = good.copy(); e[i]["pad"][1] = 1
        refused(f"prefix {i}: pad", e)
        e = good.copy(); e[i]["value"] = R.VALUE_MAX + 1
        refused(f"prefix {i}: value", e)
        e = good.copy(); e[i]["addr"][15] = 1
        refused(f"prefix {i}: address bits set past len", e)
    e = good.copy(); e[0]["addr"][1] = 0x80                  # /8 with bit 8 set
    refused("prefix 0: address bits set past len 8 (byte 1)", e)
    e = good.copy(); e[0]["addr"][0] = 0x0B; e[0]["len"] = 7   # 0000101|1
    refused("prefix 0: address bits set past len 7 (byte 0)", e)
    e = good.copy(); e[4]["addr"][4] = 1                      # version 4 past byte 3
    refused("prefix 4: address bits set past len 32 (byte 4)", e)
    e = good.copy(); e[3] = e[1]; e[3]["value"] = 9           # the same prefix, another value
    refused("prefixes 1 and 3 are the same", e)
    big = np.zeros(R.MAX_PREFIXES + 1, R.PREFIX_DTYPE)
    refused("above ZP_ROUTE_MAX_PREFIXES", big, n=R.MAX_PREFIXES + 1, nbytes=1 << 40)
    refused("null prefixes", None)
    refused("null table", good, table=None, sized=False)
    refused("table_bytes", good, nbytes=nb - 1, sized=False)
    refused("misaligned", good, table=buf.view(np.uint8)[1:], sized=False)
    assert lib.zp_route_compile(good.ctypes.data, 5, buf.ctypes.data, nb) == 0
    # the same address at another length or version is another prefix
    ok = R.encode_prefixes([("10.0.0.0/8", 1), ("10.0.0.0/9", 2), ("a00::/8", 3), ("0.0.0.0/0", 4),
                            ("::/0", 5)])
    assert lib.zp_route_table_bytes(ok.ctypes.data, 5) == HDR_BYTES + ROOT_BYTES
    assert lib.zp_route_compile(None, 0, buf.ctypes.data, nb) == 0 and \
        lib.zp_route_table_bytes(None, 0) == HDR_BYTES + ROOT_BYTES
    with pytest.raises(ValueError, match="version"):
        e = good.copy(); e[0]["version"] = 0
        R.compile_prefixes(e)


def test_device_refusals_touch_no_device(zp):
    """Every refusal returns negative with its cause named, before any HIP
    call: the pointers given are never dereferenced."""
    lib = zp._lib.hip()
    P = 4096                                             # a non-null "device pointer"
    DEST, SRC = NAMES.index("dest_addr"), NAMES.index("src_addr")

    def call(arena=P, offs=P, lens=P, recs=P, n=1000, table=P, nbytes=HDR_BYTES + ROOT_BYTES,
             col=DEST, only=None, value_of=P, mask=P, status=P):
        return lib.zp_route_device(arena, offs, lens, recs, n, table, nbytes, col, only, value_of,
                                   mask, status, None)

    def refused(what, **kw):
        assert call(**kw) < 0, what
        msg = lib.zp_last_error().decode()
        assert "zp_route_device" in msg and what in msg, (what, msg)
    refused("null records", recs=None)
    refused("null table", table=None)
    refused("null status", status=None)
    for col in (-1, 0, NAMES.index("inner_dest_addr"), NAMES.index("ip_version"), len(NAMES)):
        refused("col must be", col=col)
    refused("needs arena, offs and lens", arena=None)
    refused("needs arena, offs and lens", offs=None, col=SRC)
    refused("needs arena, offs and lens", lens=None)
    refused("2^32", n=1 << 32)
    refused("table_bytes", nbytes=HDR_BYTES + ROOT_BYTES - 1)
    refused("misaligned", table=P + 4)
    refused("misaligned", only=P + 4)
    refused("misaligned", mask=P + 4)
    refused("misaligned", status=P + 4)
    refused("misaligned", value_of=P + 2)
    words = 8 * ((1000 + 63) // 64)
    refused("mask overlaps only", only=P, mask=P)
    refused("mask overlaps only", only=P + words - 8, mask=P)
    refused("mask overlaps only", only=P, mask=P + words - 8)
    refused("null records", recs=None, only=P + words)   # adjacent is fine; the next cause is named


# ---- CPU: a body that is not a compiled one ---------------------------------

def test_corrupted_body_stays_inside_the_table(zp):
    """Random dwords behind a valid header, the table ending exactly where an
    inaccessible page begins: every lookup returns, having read nothing
    outside the table."""
    R, lib = zp.routes, zp._lib.hip()
    enc = chains(zp, [ip("10.0.0.1"), ip("2001:db8:85a3::8a2e:370:7334")])
    good = R.compile_prefixes(enc)
    nb, page = good.size, mmap.PAGESIZE
    span = (nb + page - 1) // page * page
    mm = mmap.mmap(-1, span + page)
    base = ctypes.addressof(ctypes.c_char.from_buffer(mm))
    libc = ctypes.CDLL(None, use_errno=True)
    libc.mprotect.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    assert libc.mprotect(base + span, page, 0) == 0       # PROT_NONE behind the table
    try:
        at = base + span - nb
        view = np.frombuffer((ctypes.c_uint8 * nb).from_address(at), np.uint8)
        rng = np.random.default_rng(9)
        nodes = int(good.view("<u4")[3])
        addr = np.zeros(16, np.uint8)
        look = lambda v: int(lib.zp_route_lookup_host(at, nb, addr.ctypes.data, v))
        for fill in ("random", "children", "last node", "self"):
            view[:] = good
            body = view[HDR_BYTES:].view("<u4")
            if fill == "random":
                body[:] = rng.integers(0, 1 << 32, body.size, dtype=np.uint64).astype(np.uint32)
            elif fill == "children":                      # every entry a child, most past the pool
                body[:] = 0x80000000 | rng.integers(0, 4 * nodes, body.size).astype(np.uint32)
            elif fill == "last node":                     # the deepest legal chain, at the table's end
                body[:] = 0x80000000 | (nodes - 1)
            else:                                         # node 0 points at itself: no loop
                body[:] = 0x80000000
            seen = set()
            for k in range(4000):
                addr[:] = rng.integers(0, 256, 16)
                seen.add(look(6 if k % 2 else 4))
            if fill != "random":
                assert seen == {NONE}, fill              # a walk that never meets a leaf ends with NONE
        # a header that does not describe these bytes: NONE, whatever the address
        view[:] = good
        addr[:4] = [10, 0, 0, 1]
        addr[4:] = 0
        want = int(rref.match_addrs(enc, addr[None], np.array([4]))[0][0])
        assert look(4) == want != NONE
        assert int(lib.zp_route_lookup_host(at, nb - NODE_BYTES, addr.ctypes.data, 4)) == NONE
        for word in (0, 1, 3, 4, 5):
            view[:] = good
            view.view("<u4")[word] += 1
            assert look(4) == NONE, word
    finally:
        assert libc.mprotect(base + span, page, 3) == 0


# ---- CPU: the stand-alone sanitizer program ---------------------------------

def test_host_program_under_sanitizers():
    """tests/cpp/route_host_main.c with zp_route_tab.c under
    -fsanitize=address,undefined (gcc), run as a program: the same tables,
    brute-force lookups and the corrupted-body case."""
    gcc = shutil.which("gcc")
    assert gcc, "gcc is needed"
    out = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "route_host_san")
    subprocess.run([gcc, "-std=c11", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                    "-I", os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "route_host_main.c"),
                    os.path.join(ROOT, "zero-packet_amd", "csrc", "zp_route_tab.c")], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert run.stdout.strip().endswith("route_host: OK"), run.stdout[-500:]


# ---- GPU --------------------------------------------------------------------

SENT_V, SENT_M, PAD = -7, -9, 64


def route(zp, b, table, by="dest_addr", only=None, want=("value_of", "mask"), **kw):
    """table.run into sentinel-filled buffers PAD entries longer than needed
    -> (value_of, mask as numpy; None where not wanted), asserting that
    nothing past the batch was written."""
    import torch
    da, do, dl, dr = b.device()
    n, words = b.n, (b.n + 63) // 64
    out = {"value_of": torch.full((n + PAD,), SENT_V, dtype=torch.int32, device=dev()),
           "mask": torch.full((words + PAD,), SENT_M, dtype=torch.int64, device=dev()),
           "status": torch.full((1,), -1, dtype=torch.int64, device=dev())}
    r = table.run(da, do, dl, dr, by=by, only=only, want=want, out=out, **kw)
    torch.cuda.synchronize()
    assert int(r.status[0]) == 0
    v = m = None
    if "value_of" in want:
        v = r.value_of.cpu().numpy()
        assert (v[n:] == SENT_V).all(), "value_of written past n"
        v = v[:n].view(np.uint32)
    else:
        assert r.value_of is None and (out["value_of"] == SENT_V).all()
    if "mask" in want:
        m = r.mask.cpu().numpy()
        assert (m[words:] == SENT_M).all(), "mask written past ceil(n / 64)"
        m = m[:words].view(np.uint64)
    else:
        assert r.mask is None and (out["mask"] == SENT_M).all()
    return v, m


def check_route(zp, b, enc, by="dest_addr", only=None):
    """Runs the table on the device and compares everything with route_ref;
    returns the reference (value_of, prefix)."""
    table = zp.routes.RouteTable(enc, dev())
    want, prefix = rref.match(enc, b.cols, b.packed, by, only)
    donly = to_dev(sref.mask_words(only))[0] if only is not None else None
    v, m = route(zp, b, table, by, donly)
    assert np.array_equal(v, want), np.flatnonzero(v != want)[:8]
    assert np.array_equal(m, rref.mask_words(want))
    for w in (("value_of",), ("mask",)):                 # each output alone: the other untouched
        v1, m1 = route(zp, b, table, by, donly, want=w)
        assert (v1 is None or np.array_equal(v1, want)) and \
            (m1 is None or np.array_equal(m1, rref.mask_words(want)))
    return want, prefix


def batch_table(zp, b, by, seed=1, sample=30, extra=40, short=False):
    """A table built from the batch: for a sample of its routed frames the
    address truncated to each length of interest up to a cap that cycles over
    the lengths (nested chains that end at every trie depth), and random
    prefixes that match nothing. short: lengths 0 and 1, the defaults, too."""
    rng = np.random.default_rng(seed)
    ok = rref.routed(b.packed)
    addrs, caps = [], []
    for version in (4, 6):
        idx = np.flatnonzero(ok & (b.cols["ip_version"] == version))
        idx = rng.choice(idx, min(sample, len(idx)), replace=False) if len(idx) else idx
        long = [x for x in LENS[version] if x >= 15]
        for k, i in enumerate(idx):
            addrs.append((version, bytes(b.cols[by][i])))
            caps.append(long[k % len(long)])
    enc = chains(zp, addrs, caps)
    if not short:
        enc = enc[enc["len"] > 1]
    items = []
    for k in range(extra):
        version = 4 if k % 2 else 6
        length = int(rng.choice([x for x in LENS[version] if x >= 16]))
        a = bytes(rng.integers(0, 256, 16).astype(np.uint8))
        items.append((version, length, trunc(a[:4] + bytes(12) if version == 4 else a, length), 7000 + k))
    rand = raw_prefixes(zp, items)
    hit = {int(p) for p in rref.match(rand, b.cols, b.packed, by)[1] if p >= 0}
    rand = rand[[k for k in range(len(rand)) if k not in hit]]
    assert len(rand) >= extra // 2
    return np.concatenate([enc, rand])


def assert_exercised(enc, want, prefix, versions=(4, 6), values=20):
    """From the reference alone: NONE and matched frames, many values, an
    answer from every trie depth."""
    assert (want == NONE).any() and (want != NONE).any()
    assert len(set(want[want != NONE].tolist())) >= values
    d = rref.depth(enc, prefix)
    ver = enc["version"][np.maximum(prefix, 0)]
    if 4 in versions:
        assert {1, 2, 3} <= set(d[(ver == 4) & (prefix >= 0)].tolist())
    if 6 in versions:
        assert d[(ver == 6) & (prefix >= 0)].max() >= 5


SIZES = [1, 63, 64, 65, 255, 256, 257]


def test_batch_tables_exercise_the_trie(zp, golden):
    """CPU: the tables the GPU tests build answer from every depth."""
    for cfg, versions in (("mixed", (4, 6)), ("c4", (6,)), ("c5", (4, 6)), ("c6", (4, 6))):
        b = corpus(zp, golden, cfg)
        for by in ("dest_addr", "src_addr"):
            enc = batch_table(zp, b, by)
            want, prefix = rref.match(enc, b.cols, b.packed, by)
            assert_exercised(enc, want, prefix, versions)
            assert len(enc) <= bound(enc) // NODE_BYTES


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES + ["grid+1"])
def test_sizes(zp, n):
    """Batches around the wave and tile sizes; 64-B c2 frames for one frame
    past grid x FX_BLOCK, so that some workgroup takes a second tile."""
    import torch
    cfg, values = "c3", 1
    if n == "grid+1":
        cus = torch.cuda.get_device_properties(dev()).multi_processor_count
        n, cfg, values = cus * 5 * 256 + 1, "c2", 20
    b = Batch(*zp.batch.generate_host(cfg, n, first=5))
    assert (b.recs["err"] == 0).all()
    # the table comes from the batch's first, last and middle frames
    pick = sorted({0, n - 1, n // 2, n // 3, max(n - 65, 0)} | set(range(0, n, max(n // 24, 1))))
    addrs = [(4, bytes(b.cols["dest_addr"][i])) for i in pick]
    long = [x for x in LENS[4] if x >= 15]
    enc = chains(zp, addrs, [long[k % len(long)] for k in range(len(addrs))])
    enc = enc[enc["len"] > 1]
    want, prefix = check_route(zp, b, enc)
    assert want[0] != NONE and want[n - 1] != NONE and len(set(want.tolist())) >= min(values, n)
    if n > 256:
        assert (want == NONE).any() and {1, 2, 3} <= set(rref.depth(enc, prefix).tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("by", ["dest_addr", "src_addr"])
@pytest.mark.parametrize("cfg", ["mixed", "c4", "c5", "c6"])
def test_corpora(zp, golden, cfg, by):
    """The mixed corpus and mutated c4 / c5 / c6 frames (ARP, IP-in-IP, every
    tagging, error records) against tables built from the batch."""
    b = corpus(zp, golden, cfg)
    enc = batch_table(zp, b, by)
    want, prefix = check_route(zp, b, enc, by)
    assert_exercised(enc, want, prefix, (6,) if cfg == "c4" else (4, 6))
    # with the defaults every routed frame matches; the rest stays NONE
    want, _ = check_route(zp, b, batch_table(zp, b, by, short=True), by)
    assert np.array_equal(want != NONE, rref.routed(b.packed))
    if cfg == "c6":
        F = zp.records
        flags = b.packed["flags"]
        assert ((flags & F.F_ARP) != 0).any() and ((flags & F.F_IP_IN_IP) != 0).any()


@pytest.mark.gpu
def test_frames_not_routed(zp, golden):
    """Error records, frames without an IP reader and frames whose `only`
    bit is clear give NONE and a clear mask bit; `only` from select.run."""
    b = corpus(zp, golden)
    enc = batch_table(zp, b, "dest_addr", short=True)
    ok = rref.routed(b.packed)
    err = b.recs["err"] != 0
    noip = (b.recs["err"] == 0) & (b.cols["ip_version"] == 0)
    assert err.sum() > 50 and noip.sum() > 5 and ok.sum() > 500
    rng = np.random.default_rng(2)
    want, _ = check_route(zp, b, enc)
    assert (want[err] == NONE).all() and (want[noip] == NONE).all() and (want[ok] != NONE).all()
    only = rng.random(b.n) < 0.5
    only[:64] = False                                    # a whole word clear
    want, _ = check_route(zp, b, enc, only=only)
    assert (want[~only] == NONE).all() and (want[only & ok] != NONE).all()
    # only = the mask select.run writes
    S = zp.select.Select
    sel = S(ok=True, has=("udp",))
    s = zp.select.run(*b.device(), sel, want=("mask",))
    chosen = sref.select_mask(sel.encode(), b.cols, b.packed, b.lens)
    assert 50 < chosen.sum() < ok.sum()
    table = zp.routes.RouteTable(enc, dev())
    v, m = route(zp, b, table, only=s.mask)
    want = rref.value_of(enc, b.cols, b.packed, "dest_addr", chosen)
    assert np.array_equal(v, want) and np.array_equal(m, rref.mask_words(want))
    assert np.array_equal(want != NONE, chosen & ok)


@pytest.mark.gpu
def test_table_edges(zp, golden):
    """The empty table, a default-route-only table, the aliasing pair."""
    b0 = corpus(zp, golden, "c5")
    frames = [b0.arena[int(o):int(o) + int(l)].tobytes() for o, l in zip(b0.offs, b0.lens)]
    # 10.0.0.1 -> 10.0.0.2 (ipv4_in_ipv4) and an IPv6 frame whose addresses start with 0a00:0001
    v4 = bytes.fromhex(golden["fixtures"][14]["bytes"])
    from pybuilder import internet_checksum, pseudo_header
    f = bytearray(bytes.fromhex(golden["fixtures"][5]["bytes"]))
    assert golden["fixtures"][5]["name"] == "ipv6_udp_payload"
    f[22:26] = f[38:42] = bytes([0x0A, 0, 0, 1])
    f[60:62] = b"\0\0"
    ck = internet_checksum(bytes(f[54:]), pseudo_header(bytes(f[22:38]), bytes(f[38:54]), 17, len(f) - 54))
    f[60:62] = ck.to_bytes(2, "big")
    b = Batch(*pack(frames[:300] + [bytes(f), v4] + frames[300:500]))
    assert b.recs["err"][300] == 0 and b.recs["err"][301] == 0
    assert b.cols["ip_version"][300] == 6 and b.cols["ip_version"][301] == 4
    R = zp.routes
    want, _ = check_route(zp, b, R.encode_prefixes([]))
    assert (want == NONE).all()
    for by in ("dest_addr", "src_addr"):
        want, _ = check_route(zp, b, R.encode_prefixes([("0.0.0.0/0", 9)]), by)
        assert np.array_equal(want == 9, rref.routed(b.packed) & (b.cols["ip_version"] == 4))
        assert (want[b.cols["ip_version"] != 4] == NONE).all()
        want, _ = check_route(zp, b, R.encode_prefixes([("a00:1::/32", 66), ("10.0.0.0/8", 44)]), by)
        assert want[300] == 66 and want[301] == 44
        want, _ = check_route(zp, b, R.encode_prefixes([("a00:1::/32", 66)]), by)
        assert want[300] == 66 and want[301] == NONE
        want, _ = check_route(zp, b, R.encode_prefixes([("10.0.0.0/8", 44), ("::/0", 5)]), by)
        assert want[300] == 5 and want[301] == 44


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["gaps", "reverse", "shuffled", "dup"])
def test_layouts(zp, golden, layout):
    from test_gpu_parity import layout_batch
    b0 = corpus(zp, golden)
    frames = [b0.arena[int(o):int(o) + int(l)].tobytes() for o, l in zip(b0.offs, b0.lens)][:900]
    b = Batch(*layout_batch(frames, layout))
    enc = batch_table(zp, b, "dest_addr")
    want, prefix = check_route(zp, b, enc)
    assert_exercised(enc, want, prefix, values=15)


def raw(zp, b, table_t, nbytes, n=None):
    """zp_route_device into sentinel buffers -> (rc, status, value_of, mask)."""
    import torch
    da, do, dl, dr = b.device()
    n = b.n if n is None else n
    value_of = torch.full((n + PAD,), SENT_V, dtype=torch.int32, device=dev())
    mask = torch.full(((n + 63) // 64 + PAD,), SENT_M, dtype=torch.int64, device=dev())
    status = torch.full((1,), -1, dtype=torch.int64, device=dev())
    rc = zp._lib.hip().zp_route_device(
        da.data_ptr(), do.data_ptr(), dl.data_ptr(), dr.data_ptr(), n, table_t.data_ptr(), nbytes,
        NAMES.index("dest_addr"), None, value_of.data_ptr(), mask.data_ptr(), status.data_ptr(), None)
    torch.cuda.synchronize()
    return rc, int(status[0]), value_of.cpu().numpy(), mask.cpu().numpy()


@pytest.mark.gpu
def test_status_refuses_a_wrong_table(zp, golden):
    """The kernel checks the header before anything else: a table passed with
    another table's size, or a zeroed one, gives status 1 and leaves every
    output as it was."""
    import torch
    b = corpus(zp, golden, "c5")
    enc = batch_table(zp, b, "dest_addr")
    t = zp.routes.RouteTable(enc, dev())
    small = zp.routes.RouteTable(enc[enc["len"] <= 24], dev())
    assert small.table.numel() < t.table.numel()

    def untouched(res):
        rc, status, v, m = res
        assert rc == 0 and status == 1 and (v == SENT_V).all() and (m == SENT_M).all()
    untouched(raw(zp, b, t.table, small.table.numel()))            # another table's size
    untouched(raw(zp, b, t.table, t.table.numel() - 1024))
    untouched(raw(zp, b, torch.zeros_like(t.table), t.table.numel()))   # never written
    rc, status, v, m = raw(zp, b, t.table, t.table.numel())        # and the right call goes through
    assert rc == 0 and status == 0
    assert np.array_equal(v[:b.n].view(np.uint32), rref.value_of(enc, b.cols, b.packed))
    assert (v[b.n:] == SENT_V).all()
    # the facade raises on it
    t.table = torch.cat([t.table, torch.zeros(1024, dtype=torch.uint8, device=dev())])
    with pytest.raises(RuntimeError, match="status 1"):
        t.run(*b.device())
    # n == 0 writes status only
    rc, status, v, m = raw(zp, b, small.table, small.table.numel(), n=0)
    assert rc == 0 and status == 0 and (v == SENT_V).all() and (m == SENT_M).all()
    # CPU tensors are refused by the facade
    with pytest.raises(RuntimeError, match="device tensors"):
        small.run(b.device()[0].cpu(), *b.device()[1:])


@pytest.mark.gpu
@pytest.mark.parametrize("by", ["dest_addr", "src_addr"])
def test_agrees_with_classify(zp, golden, by):
    """A table of at most 256 prefixes as a RuleTable, one rule per prefix in
    descending length: rule_of mapped through the values equals value_of."""
    b = corpus(zp, golden, "c5")
    enc = batch_table(zp, b, by, sample=8, extra=10, short=True)
    assert 50 < len(enc) <= 256
    order = np.argsort(-enc["len"].astype(np.int64), kind="stable")
    S = zp.select.Select
    rules = []
    for k in order:
        p = enc[k]
        nb = 4 if p["version"] == 4 else 16
        net = ipaddress.ip_network((bytes(p["addr"][:nb]), int(p["len"])))
        rules.append(S(ok=True).where(by, prefix=str(net)).where("ip_version", eq=int(p["version"])))
    c = zp.classify.RuleTable(rules, dev()).run(*b.device(), want=("rule_of",))
    rule = c.rule_of.cpu().numpy().view(np.uint32)
    mapped = np.where(rule == NONE, NONE, enc["value"][order][np.minimum(rule, len(enc) - 1)])
    v, _ = route(zp, b, zp.routes.RouteTable(enc, dev()), by)
    assert np.array_equal(v, mapped.astype(np.uint32))
    assert len(set(v.tolist())) >= 10 and (v == NONE).any()


@pytest.mark.gpu
def test_forwarding_pipeline(zp, golden):
    """route on dest_addr -> hop_mac[value_of] -> columns.rewrite of dest_mac
    and ttl - 1 on the matched frames -> reparse: the records are unchanged
    and the extracted MACs are the written ones."""
    import torch
    b = Batch(*zp.batch.generate_host("c5", 1500, first=3))
    da, do, dl, dr = [t.clone() for t in b.device()]
    enc = batch_table(zp, b, "dest_addr")
    enc["value"] = np.arange(len(enc))                    # next-hop indices
    table = zp.routes.RouteTable(enc, dev())
    r = table.run(da, do, dl, dr)
    want = rref.value_of(enc, b.cols, b.packed)
    hit = want != NONE
    assert np.array_equal(r.value_of.cpu().numpy().view(np.uint32), want) and 20 < hit.sum() < b.n
    hop_mac = torch.tensor([[2, 0, (k >> 8) & 255, k & 255, 0xAA, 0x55] for k in range(len(enc))],
                           dtype=torch.uint8, device=dev())
    cols = zp.columns.extract(da, do, dl, dr, names=["dest_mac", "ttl"])
    matched = r.value_of != -1
    new_mac = torch.where(matched[:, None], hop_mac[r.value_of.clamp(min=0).long()], cols["dest_mac"])
    new_ttl = torch.where(matched, cols["ttl"] - 1, cols["ttl"])
    zp.columns.rewrite(da, do, dl, dr, {"dest_mac": new_mac, "ttl": new_ttl})
    recs2, _ = zp.batch.parse_batch(da, do, dl)
    got = zp.columns.extract(da, do, dl, recs2, names=["dest_mac", "ttl", "dest_addr"])
    torch.cuda.synchronize()
    assert torch.equal(recs2.view(torch.uint8).reshape(-1), dr.view(torch.uint8).reshape(-1))
    mac = got["dest_mac"].cpu().numpy()
    assert np.array_equal(mac[hit], hop_mac.cpu().numpy()[want[hit].astype(np.int64)])
    assert np.array_equal(mac[~hit], b.cols["dest_mac"][~hit])
    assert np.array_equal(got["ttl"].cpu().numpy()[hit], (b.cols["ttl"][hit] - 1).astype(np.uint8))
    assert np.array_equal(got["dest_addr"].cpu().numpy(), b.cols["dest_addr"])


@pytest.mark.gpu
def test_mask_feeds_the_flow_table(zp, golden):
    """Blocklist accounting: route on src_addr, its mask into flows.aggregate."""
    import flow_ref
    from test_flows import FIVE, mixed, opts_of, read, run
    b = mixed(zp, golden)
    enc = batch_table(zp, b, "src_addr", sample=60)
    want = rref.value_of(enc, b.cols, b.packed, "src_addr")
    m = want != NONE
    assert 30 < m.sum() < flow_ref.keyed(b.packed).sum()
    r = zp.routes.RouteTable(enc, dev()).run(*b.device(), by="src_addr", want=("mask",))
    t = run(zp, b, mask=r.mask)
    count, flows, fo = read(t, b.n, b.n)
    wfo, went, wcnt = flow_ref.aggregate(b.cols, b.packed, b.lens, opts_of(FIVE, b.n), m)
    assert count == wcnt and np.array_equal(fo, wfo)
    assert flows[:wcnt[0]].tobytes() == went.tobytes()


@pytest.mark.gpu
def test_two_tables_in_a_graph(zp, golden):
    """run(check=False) twice with different tables, captured in one graph
    and replayed once."""
    import torch
    b = corpus(zp, golden, "c5")
    da, do, dl, dr = b.device()
    encs = [batch_table(zp, b, "dest_addr", seed=1), batch_table(zp, b, "src_addr", seed=2)]
    tables = [zp.routes.RouteTable(e, dev()) for e in encs]
    outs = [{"value_of": torch.full((b.n,), SENT_V, dtype=torch.int32, device=dev()),
             "mask": torch.zeros((b.n + 63) // 64, dtype=torch.int64, device=dev()),
             "status": torch.full((1,), -1, dtype=torch.int64, device=dev())} for _ in tables]
    bys = ["dest_addr", "src_addr"]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                        # warm up outside the capture
        for t, o, by in zip(tables, outs, bys):
            t.run(da, do, dl, dr, by=by, out=o, check=False)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for o in outs:
        o["value_of"].fill_(SENT_V)
        o["status"].fill_(-1)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = [t.run(da, do, dl, dr, by=by, out=o, check=False)
               for t, o, by in zip(tables, outs, bys)]
    g.replay()
    torch.cuda.synchronize()
    for r, e, by in zip(res, encs, bys):
        want = rref.value_of(e, b.cols, b.packed, by)
        assert int(r.status[0]) == 0
        assert np.array_equal(r.value_of.cpu().numpy().view(np.uint32), want)
        assert np.array_equal(r.mask.cpu().numpy().view(np.uint64), rref.mask_words(want))
    assert not np.array_equal(res[0].value_of.cpu().numpy(), res[1].value_of.cpu().numpy())
