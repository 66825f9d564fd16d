"""L4 word sums on a multiple of 2^32 (tests/wrapframes.py): the parse and the
header rewrite against the oracle where the reference's wrapping u32 sum
(checksum.rs:5-29) and arithmetic mod 65535 part ways.

CPU: every fixture is what it claims (exact sum, wrap counts before and after
the intended write, the oracle's verdict), and the rewrite fixtures marked as
crossing are exactly those on which an update from the changed words alone
(RFC 1624) differs from the writers' full recompute. ZP_REWRITE_EXACT_L4_BYTES
is read from the header and its derivation re-checked.
GPU: the parse fixtures through the plain, code and fused kernels at both
arena parities, records and columns equal to the oracle's; the rewrite
fixtures through run_rewrite (bytes == rewrite_ref, the oracle re-parses the
output to the same records).
"""
import os
import re

import numpy as np
import pytest

import oracle as orc
import wrapframes as wf
from fuzzfix import repair
from rewrite_ref import WRITABLE, rewrite_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_V6_L4 = 35                                   # ZP_ERR_IPV6_L4_CHECKSUM
PARSE = sorted(wf.parse_fixtures())
REWRITE = sorted(wf.rewrite_fixtures())
CROSSING = {"W1", "W1_ffff", "W2", "W4", "W5", "W6", "W8_tunnel"}


def exact_bytes():
    h = open(os.path.join(ROOT, "include", "zero_packet.h")).read()
    return int(re.search(r"#define\s+ZP_REWRITE_EXACT_L4_BYTES\s+(\d+)u?\b", h).group(1))


def sum_bound(n):
    """The largest exact sum of an L4 slice of n bytes with its pseudo-header:
    every word 0xFFFF (an odd last byte fills a word's high half), two IPv6
    addresses of 0xFFFF words, protocol <= 255, the length itself."""
    return (n + 1) // 2 * 0xFFFF + 16 * 0xFFFF + 255 + n


# ---- CPU -----------------------------------------------------------------------

def test_exact_threshold_derivation():
    n = exact_bytes()
    assert sum_bound(n - 1) < 1 << 32 <= sum_bound(n)
    assert all(sum_bound(k) <= sum_bound(k + 1) for k in range(n - 64, n + 64))
    # every fixture lies above it, and the suite's other rewrite frames below
    assert wf.L_ONE >= n and wf.L_TWO >= n
    # an all-0xFF slice one byte shorter cannot be built up to 2^32
    with pytest.raises(AssertionError):
        wf.wrap_frame(wf.TCP, 1 << 32, n - 1)


def test_fold_restates_the_oracle():
    """wrapframes' integer arithmetic and the oracle's internet_checksum agree
    on wrapped accumulators (zpo_internet_checksum takes the u32 acc)."""
    for s in (1, 0xFFFF, 0x10000, 0xFFFFFFFF, 0xFFFF0000, 0x12345678):
        assert wf.fold(s) == orc.internet_checksum(b"", s)
    assert wf.stored_for(1 << 32) == 0xFFFF and not wf.accepts(1 << 32)
    assert wf.accepts((1 << 32) - 1) and wf.accepts((1 << 32) + 0xFFFF)
    assert not wf.accepts((1 << 32) + 0xFFFE)


@pytest.mark.parametrize("name", PARSE)
def test_parse_fixture_is_what_it_claims(name):
    frame, total, ok = wf.parse_fixtures()[name]
    err, rec, _ = orc.parse_one(frame)
    assert err == (0 if ok else ERR_V6_L4), (name, err)
    odd = name.endswith("_odd")
    assert (len(frame) - 54) % 2 == int(odd)
    wraps = {"ffffffff": 0, "wrap_ffff": 1, "two32": 1, "wrap_fffe": 1, "twice": 2}
    base = name.replace("_odd", "").replace("_bad", "")
    assert total >> 32 == wraps[base]
    if ok:                                          # the stored checksum is the writers'
        assert repair(frame) == frame
    # where the two arithmetics part: a verdict taken mod 65535 is the other one
    if base in ("wrap_ffff", "wrap_fffe") and "_bad" not in name:
        assert (total % 65535 == 0) != ok


def fixture_batch(name):
    """(frames, index of the fixture's frame, its WrapFrame, writes, wraps)."""
    w, writes, wraps = wf.rewrite_fixtures()[name]
    if name == "W6":
        near = edge_neighbour()
        return [near, w.frame, near], 1, w, writes, wraps
    return [w.frame], 0, w, writes, wraps


def edge_neighbour():
    from test_rewrite import _eth, _ip4, _udp
    f = repair(_eth(0x0800) + _ip4(17, _udp(7, 9, bytes(22))))
    assert len(f) == 64
    return f


def fixture_columns(name, arena, offs, lens, orec):
    """The numpy columns of a fixture: the extracted values, the fixture's
    writes at its own frame."""
    frames, k, w, writes, _ = fixture_batch(name)
    old = orc.columns(arena, offs, lens, orec)
    if writes == "identity":
        return {c: old[c].copy() for c in WRITABLE}
    cols = {c: old[c].copy() for c in writes}
    for c, v in writes.items():
        cols[c][k] = np.frombuffer(v, np.uint8) if isinstance(v, bytes) else v
    return cols


def rfc1624(old, new, w):
    """The checksum an update from the changed words alone stores (RFC 1624
    eqn. 3 over the pseudo-header addresses and the L4 header, end-around
    carry, 0 counted as 0xFFFF): rw_checksum of zp_rewrite.h restated."""
    t = ~w.stored(old) & 0xFFFF
    for x in list(range(w.ip + 8, w.ip + 40, 2)) + list(range(w.l4, w.l4 + 20, 2)):
        if x != w.ck:
            t += (~((old[x] << 8) | old[x + 1]) & 0xFFFF) + ((new[x] << 8) | new[x + 1])
    while t >> 16:
        t = (t & 0xFFFF) + (t >> 16)
    return ~(t or 0xFFFF) & 0xFFFF


@pytest.mark.parametrize("name", REWRITE)
def test_rewrite_fixture_is_what_it_claims(name):
    from test_gpu_parity import pack
    frames, k, w, writes, wraps = fixture_batch(name)
    arena, offs, lens = pack(frames, base_pad=1 if name == "W6" else 0)
    orec, oext = orc.parse_batch(arena, offs, lens)
    assert (orec["err"] == 0).all(), orec["err"]
    assert len(w.frame) - w.l4 >= exact_bytes()
    cols = fixture_columns(name, arena, offs, lens, orec)
    one = {c: (v[k].tobytes() if v.ndim > 1 else int(v[k])) for c, v in cols.items()}
    new, applied = rewrite_ref(w.frame, orec[k], oext[:, k], one)
    assert (w.s0() >> 32, w.s0(new) >> 32) == wraps, (name, hex(w.s0()), hex(w.s0(new)))
    assert w.stored(new) == wf.stored_for(w.s0(new))          # rewrite_ref wraps as the writers do
    nerr, nrec, next_ = orc.parse_one(new)
    assert nerr == 0 and orc.pack(nrec, next_).tobytes() == \
        orc.pack(orec[k], oext[:, k]).tobytes()
    if writes == "identity":
        assert new == w.frame and not any(applied.values())
        return
    assert new != w.frame
    # RFC 1624 stores another checksum exactly where the sum crosses 2^32,
    # and the oracle rejects that frame
    inc = bytearray(new)
    inc[w.ck:w.ck + 2] = rfc1624(w.frame, new, w).to_bytes(2, "big")
    assert (bytes(inc) != new) == (name in CROSSING), name
    assert (wraps[0] != wraps[1]) == (name in CROSSING)
    if name in CROSSING:
        assert orc.parse_one(bytes(inc))[0] == ERR_V6_L4
    if name == "W1":                                           # the issue's figures
        assert w.stored() == 0x00FF and w.stored(new) == 0xFF00 and \
            rfc1624(w.frame, new, w) == 0xFEFF
    if name == "W1_ffff":
        assert w.stored(new) == 0x0101 and rfc1624(w.frame, new, w) == 0x0100


# ---- GPU -----------------------------------------------------------------------

from test_gpu_paths import slots  # noqa: E402,F401  (a fixture)


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("path", ["plain", "codes", "fused"])
def test_gpu_parse_wrap_boundary(zp, slots, path, shift):
    from test_gpu_paths import run_path, tight_pack
    fx = wf.parse_fixtures()
    arena, offs, lens = tight_pack([fx[k][0] for k in PARSE])
    want, wext = orc.parse_batch(arena, offs, lens)
    assert [int(e) for e in want["err"]] == [0 if fx[k][2] else ERR_V6_L4 for k in PARSE]
    packed = orc.pack(want, wext).view(np.uint8).reshape(-1, 8)
    rec, ext, cols = run_path(zp, slots, path, arena, offs, lens, base_shift=shift)
    bad = np.nonzero((rec.view(np.uint8).reshape(-1, 8) != packed).any(1))[0]
    assert bad.size == 0, ("records differ", [PARSE[i] for i in bad], rec[bad], want[bad])
    assert zp.records.ext_match(ext, wext, want)
    if cols is not None:
        wcols = orc.columns(arena, offs, lens, want)
        for name, v in wcols.items():
            assert np.array_equal(cols[name], v), name


@pytest.mark.gpu
@pytest.mark.parametrize("name", REWRITE)
def test_gpu_rewrite_wrap_boundary(zp, name):
    """W1, W1_ffff, W2, W4, W5, W6 and W8_tunnel move the sum across 2^32: the
    update from the changed words alone (rw_checksum) would store a checksum
    the parse rejects (W1: 0xFEFF for 0xFF00), so the kernel has to sum these
    slices in full; W1_below, W3 and W7 do not cross."""
    from test_gpu_parity import pack
    from test_rewrite import run_rewrite
    frames, k, w, writes, _ = fixture_batch(name)
    arena, offs, lens = pack(frames, base_pad=1 if name == "W6" else 0)
    orec, _ = orc.parse_batch(arena, offs, lens)
    cols = fixture_columns(name, arena, offs, lens, orec)
    got, changed, _ = run_rewrite(zp, arena, offs, lens, cols)
    if writes == "identity":
        assert np.array_equal(got, arena)
    else:
        assert any(changed[c][k] for c in writes)
