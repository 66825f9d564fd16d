"""The adversarial parity cases through every kernel that reads frames.

parse_tiles<> (zp_parse.hip) is three device kernels, and zp_columns_kernel
(zp_fields.hip) reads frames on its own. Each case below runs on four paths:

  plain        zp_parse_kernel (record codes off): the control
  codes        zp_parse_slots_kernel + zp_rec_expand_kernel (record codes
               always), into a records buffer pre-filled with 0xFF: byte 3
               of every tile then reads as a code tile unless the parse
               stored records there
  fused        zp_parse_columns_kernel, every column into buffers pre-filled
               with 0xA5 (an entry the kernel forgets keeps the fill)
  split_codes  the code kernels, then zp_columns_kernel on the same stream

Expected values come from the CPU oracle alone: records byte for byte, the
flagged extension chains, and every column entry. The frames and the oracle's
results of a case are built once per module; the conditions that make a case
worth running (which codes, cuts and errors occur) are asserted on the
oracle's records when the case is built, and the CPU tests build the
constructed cases, so a mis-built case fails before any GPU run.
"""
import functools

import numpy as np
import pytest

import oracle as orc
import stackgen as sg
from test_columns import getter_columns
from test_gpu_parity import LAYOUTS
from test_record_slots import rec_code

PATHS = ["plain", "codes", "fused", "split_codes"]


# ---- the runner -------------------------------------------------------------

def dev():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture
def slots(zp):
    lib = zp._lib.hip()
    prev = lib.zp_set_record_slots(0)
    yield lambda mode: lib.zp_set_record_slots(mode)
    lib.zp_set_record_slots(prev)


def run_path(zp, slots, path, arena, offs, lens, base_shift=0):
    """One batch through one path -> (records, ext, columns or None) as numpy
    (records_to_numpy's forms; columns {name: array})."""
    import torch
    d = dev()
    arena = np.ascontiguousarray(arena, np.uint8)
    n = len(offs)
    a = torch.zeros(len(arena) + base_shift, dtype=torch.uint8, device=d)   # tight arena end
    a[base_shift:] = torch.from_numpy(arena).to(d)
    o = torch.from_numpy(np.asarray(offs).astype(np.int64) + base_shift).to(d)
    l_ = torch.from_numpy(np.asarray(lens, np.uint32).astype(np.int32)).to(d)
    filled = lambda: torch.full((n, 8), 0xFF, dtype=torch.uint8, device=d)
    cols = None
    if path == "plain":
        slots(2)
        r, e = zp.batch.parse_batch(a, o, l_)
    elif path == "codes":
        slots(1)
        r, e = zp.batch.parse_batch(a, o, l_, records=filled())
    elif path in ("fused", "split_codes"):
        slots(1 if path == "split_codes" else 2)
        out = {}
        for name, dt, k in zp.columns.COLUMNS:
            buf = torch.full((n * zp.columns.width(name),), 0xA5, dtype=torch.uint8, device=d)
            out[name] = buf.view(dt).reshape((n, k) if k > 1 else (n,))
        r, e, c = zp.columns.parse_with_columns(
            a, o, l_, records=filled(), out=out,
            mode="fused" if path == "fused" else "split")
        assert sorted(c) == sorted(zp.columns.NAMES)
        torch.cuda.synchronize()
        cols = {name: t.cpu().numpy() for name, t in c.items()}
    else:
        raise ValueError(path)
    torch.cuda.synchronize()
    rec, ext = zp.batch.records_to_numpy(r, e)
    return rec, ext, cols


# ---- cases --------------------------------------------------------------------

class Batch:
    """Descriptors over an arena with the oracle's records, chains and columns."""

    def __init__(self, arena, offs, lens, shifts=(0,), tag=""):
        self.arena = np.ascontiguousarray(arena, np.uint8)
        self.offs = np.ascontiguousarray(offs).astype(np.uint64)
        self.lens = np.ascontiguousarray(lens).astype(np.uint32)
        self.shifts, self.tag = tuple(shifts), tag
        self.want, self.wext = orc.parse_batch(self.arena, self.offs, self.lens)
        self.packed = orc.pack(self.want, self.wext)
        self.cols = orc.columns(self.arena, self.offs, self.lens, self.want)

    def prefix(self, n, shifts=None, tag=""):
        """The first n descriptors, over an arena cut at their last byte."""
        b = object.__new__(Batch)
        b.offs, b.lens = self.offs[:n].copy(), self.lens[:n].copy()
        end = int((b.offs + b.lens).max()) if n else 0
        b.arena = self.arena[:end].copy()
        b.shifts, b.tag = tuple(shifts if shifts is not None else self.shifts), tag
        b.want, b.wext, b.packed = self.want[:n], self.wext[:, :n], self.packed[:n]
        b.cols = {k: v[:n] for k, v in self.cols.items()}
        return b

    def codes(self):
        """The record code of every oracle record (0: none)."""
        pairs, inv = np.unique(self.packed, return_inverse=True)
        c = np.array([rec_code(int(p["flags"]), int(p["offs"])) for p in pairs], np.int64)
        return c[inv.reshape(-1)] if len(pairs) else np.zeros(0, np.int64)


def frames_of(arena, offs, lens):
    return [arena[int(o):int(o) + int(l)].tobytes() for o, l in zip(offs, lens)]


def tight_pack(frames):
    """Frames back to back, the arena ending at the last frame's last byte."""
    from test_gpu_parity import pack
    arena, offs, lens = pack(frames)
    return arena[:int(offs[-1] + lens[-1])], offs, lens


@functools.lru_cache(maxsize=None)
def long_frames():
    """(jumbo list, word-sum list, far-L4 cases): built once, their checksums
    are Python loops over up to 300,000 B."""
    from test_gpu_parity import jumbo_frames, word_sum_frames
    from test_l4_far import _cases
    return jumbo_frames(), word_sum_frames(), _cases()


def case_fuzz_raw(zp, golden):
    from test_gpu_parity import fuzz_frames, pack
    b = Batch(*pack(fuzz_frames(zp, golden, 20000, 7)), shifts=(5,))
    assert len(np.unique(b.want["err"])) >= 18
    return [b]


def case_fuzz_repaired(zp, golden):
    """10,000 frames: refilling the checksums in Python is what this case
    costs (20,000 took longer to build than test_fuzz_gpu_vs_oracle runs)."""
    from test_gpu_parity import fuzz_frames, pack
    b = Batch(*pack(fuzz_frames(zp, golden, 10000, 11, repair_p=0.7)), shifts=(0, 3))
    assert (b.want["err"] == 0).mean() > 0.4
    return [b]


_LAYOUT_FRAMES = []


def case_layout(layout):
    def build(zp, golden):
        from test_gpu_parity import fuzz_frames, layout_batch
        if not _LAYOUT_FRAMES:                           # one frame list for the five layouts
            _LAYOUT_FRAMES.append(fuzz_frames(zp, golden, 5000, 11))
        return [Batch(*layout_batch(_LAYOUT_FRAMES[0], layout))]
    return build


def case_truncations(zp, golden):
    """A c3 frame, a c4 frame with two or more extension headers and a tagged
    c5 IP-in-IP frame, each cut at every length 0..min(len, 200)."""
    R = zp.records
    bases = []
    for cfg, keep in (
            ("c3", lambda r: True),
            ("c4", lambda r: bin((int(r["flags"]) >> 12) & 0x3F).count("1") >= 2),
            ("c5", lambda r: int(r["flags"]) & R.F_IP_IN_IP and int(r["eth_len"]) > 14)):
        a, o, l_ = zp.batch.generate_host(cfg, 256, first=42)
        rec, _ = orc.parse_batch(a, o, l_)
        assert (rec["err"] == 0).all()
        fit = [i for i in range(len(rec)) if keep(rec[i])]
        # the longest frame within the 200 cuts, so that the last cut is the
        # whole, accepted frame (else the shortest)
        i = max((i for i in fit if l_[i] <= 200), key=lambda i: l_[i],
                default=min(fit, key=lambda i: l_[i]))
        bases.append(a[int(o[i]):int(o[i] + l_[i])].tobytes())
    frames = [f[:k] for f in bases for k in range(0, min(len(f), 200) + 1)]
    b = Batch(*tight_pack(frames))
    assert int(b.offs[-1] + b.lens[-1]) == len(b.arena)
    assert (b.want["err"] == 0).sum() >= 2 and len(np.unique(b.want["err"])) >= 4
    return [b]


def case_long_frames(zp, golden):
    from test_gpu_parity import pack
    from test_oracle_golden import ERR
    jumbo, word_sum, far = long_frames()
    b = Batch(*pack(jumbo + word_sum + [f for f, _ in far]), shifts=(0, 1))
    assert set(np.unique(b.want["err"])) >= {0, ERR["IPV6_L4_CHECKSUM"]}
    n_far = sum(l4 > zp.records.L4_NEAR_MAX for _, l4 in far)
    assert n_far >= 1 and zp.records.is_far(b.packed).sum() == n_far
    return [b]


def case_min_flips(zp, golden):
    """Tiles of 64-B frames (c1) with 60 single-bit flips, a ragged last tile."""
    from test_gpu_parity import pack
    a, o, l_ = zp.batch.generate_host("c1", 64 * 300 + 17, first=99)
    a = a.copy()
    assert (l_ == 64).all()
    rng = np.random.default_rng(5)
    for i in rng.choice(len(o), 60, replace=False):
        a[int(o[i]) + int(rng.integers(0, 64))] ^= np.uint8(1 << int(rng.integers(0, 8)))
    b = Batch(*pack(frames_of(a, o, l_)), shifts=(0, 1, 2, 3, 7, 13))
    assert 10 <= int((b.want["err"] != 0).sum()) <= 60
    return [b]


def case_min_prefixes(zp, golden):
    a, o, l_ = zp.batch.generate_host("c1", 65, first=7)
    whole = Batch(a, o, l_)
    assert (whole.want["err"] == 0).all() and (l_ == 64).all()
    return [whole.prefix(n, shifts=(0, 11), tag=f"n={n}") for n in (1, 5, 63, 64, 65)]


def case_min_same(zp, golden):
    """One tile whose 64 descriptors name the same frame."""
    a, o, l_ = zp.batch.generate_host("c1", 65, first=7)
    b = Batch(a, np.full(64, o[3], np.uint64), l_[:64])
    assert (b.want["err"] == 0).all()
    return [b]


def case_mostly_coded(zp, golden):
    """c3 with one frame in 64 mutated as test_common_frame_path_mutations
    mutates: about (1 - 1/64)^64 = 0.37 of the tiles keep their codes."""
    a, o, l_ = zp.batch.generate_host("c3", 64 * 200 + 63, first=4242)
    a = a.copy()
    rng = np.random.default_rng(11)
    for i in np.nonzero(rng.random(len(o)) < 1 / 64)[0]:
        k = int(rng.integers(0, 4))
        if k == 0:                              # a header byte (Ethernet, IPv4, L4 words)
            j = int(rng.choice([12, 13, 14, 16, 17, 22, 23, 24, 25, 34, 35, 38, 39, 46, 47]))
        elif k == 1:                            # any byte of the first 64
            j = int(rng.integers(0, 64))
        else:                                   # any byte (the L4 checksum)
            j = int(rng.integers(0, int(l_[i])))
        a[int(o[i]) + j] ^= np.uint8(1 << int(rng.integers(0, 8)))
    b = Batch(a, o, l_, shifts=(0, 3))
    full = len(o) // 64
    coded = (b.codes()[:full * 64].reshape(full, 64) != 0).all(1).mean()
    assert 0.2 <= coded <= 0.6, coded
    assert int((b.want["err"] != 0).sum()) >= 100
    return [b]


def case_every_code(zp, golden):
    """Every record code as a whole tile, mixed-code tiles, one anomaly per
    tile at the lanes the expansion reads, a ragged tail; the whole batch and
    prefixes that end on either side of the expansion's 16- and 64-tile
    boundaries."""
    from test_gpu_parity import _jumbo_ipv6, pack
    _, _, far = long_frames()
    rng = np.random.default_rng(77)
    giant = _jumbo_ipv6(70001, rng, False, 58)
    giant_ok = _jumbo_ipv6(70001, rng, True, 58)
    frames, intended = sg.code_batch(rng, giant, far[1][0], giant_ok)
    whole = Batch(*tight_pack(frames), tag="whole")
    codes = whole.codes()
    assert (codes == intended).all(), np.nonzero(codes != intended)[0][:5]
    assert len(frames) == 94 * 64 + 37
    tiles = codes[:94 * 64].reshape(94, 64)
    single = {int(t[0]) for t in tiles if t[0] and (t == t[0]).all()}
    assert single == set(sg.valid_codes()) and len(single) == 33
    first = 66
    for k in range(len(sg.ANOMALIES) * len(sg.ANOMALY_LANES)):
        t = tiles[first + k]
        lane = sg.ANOMALY_LANES[k % len(sg.ANOMALY_LANES)]
        assert (t == 0).sum() == 1 and t[lane] == 0, (k, lane)
    assert zp.records.is_far(whole.packed).sum() == len(sg.ANOMALY_LANES)
    assert (tiles[first + 27] != 0).all() and whole.lens[(first + 27) * 64 + 3] == 70001
    assert (codes[94 * 64:] != 0).all()
    return [whole] + [whole.prefix(n, tag=f"n={n}") for n in sg.CODE_PREFIXES]


def _cuts(field, wlen, mask):
    """Bytes of a field inside the window, where the window end cuts it."""
    c = wlen[mask].astype(np.int64) - field[mask].astype(np.int64)
    return set(c[(c >= 1) & (c <= 15)].tolist())


def case_window_edge(zp, golden):
    """L4 and inner IP headers on and past the end of the parse window, at
    every start alignment mod 16: field reads that straddle the window edge."""
    R = zp.records
    fam = sg.window_families(np.random.default_rng(2025))
    frames = fam["A"] + fam["B"] + fam["C"]
    arena, offs, lens, idx = sg.place_aligned(frames)
    b = Batch(arena, offs, lens)
    b.frames, b.frame_idx = frames, idx
    assert len(fam["A"]) + len(fam["B"]) == 288 and len(offs) == 16 * len(frames)
    assert set((offs % 16).tolist()) == set(range(16))
    w = b.want
    assert (w["err"] == 0).all()
    wlen = 112 - (offs % 16).astype(np.int64)
    l4, inner, flags = w["l4_off"].astype(np.int64), w["inner_off"].astype(np.int64), w["flags"]
    tcp = (flags & R.F_TCP) != 0
    ports = (flags & (R.F_TCP | R.F_UDP)) != 0
    ipip = (flags & R.F_IP_IN_IP) != 0
    in6 = ipip & ((flags & R.F_IP_IN_IP_V6) != 0)
    in4 = ipip & ~in6
    for d in (4, 8):                                     # tcp_seq, tcp_ack
        assert {1, 2, 3} <= _cuts(l4 + d, wlen, tcp), d
    assert 1 in _cuts(l4, wlen, ports)                   # src_port
    for d in (12, 16):                                   # TCP offset/flags word, checksum
        assert 1 in _cuts(l4 + d, wlen, tcp), d
    for d in (8, 24):                                    # inner IPv6 src, dest
        assert set(range(1, 16)) <= _cuts(inner + d, wlen, in6), d
    for d in (12, 16):                                   # inner IPv4 src, dest
        assert {1, 2, 3} <= _cuts(inner + d, wlen, in4), d
    assert int((ipip & (inner >= wlen)).sum()) >= 100
    assert int((l4 >= wlen).sum()) >= 1000               # L4 reader wholly past the window
    for name, col in b.cols.items():
        assert (name == "arp_oper") != bool(col.any()), name
    return [b]


CASES = {"fuzz_raw": case_fuzz_raw, "fuzz_repaired": case_fuzz_repaired,
         **{"layout_" + x: case_layout(x) for x in LAYOUTS},
         "truncations": case_truncations, "long_frames": case_long_frames,
         "min_flips": case_min_flips, "min_prefixes": case_min_prefixes,
         "min_same": case_min_same, "mostly_coded": case_mostly_coded,
         "every_code": case_every_code, "window_edge": case_window_edge}
_BUILT = {}


def get_case(zp, golden, name):
    if name not in _BUILT:
        _BUILT[name] = CASES[name](zp, golden)
    return _BUILT[name]


def check(zp, b, path, shift, got, gext, cols):
    where = (path, b.tag, f"shift {shift}")
    g = got.view(np.uint8).reshape(-1, 8)
    w = b.packed.view(np.uint8).reshape(-1, 8)
    assert g.shape == w.shape, where
    diff = np.nonzero((g != w).any(1))[0]
    assert len(diff) == 0, (where, f"{len(diff)} records differ; first {diff[:5]}",
                            got[diff[:3]], b.packed[diff[:3]])
    assert zp.records.ext_match(gext, b.wext, b.want), where
    assert (cols is not None) == (path in ("fused", "split_codes"))
    if cols is not None:
        for name in zp.columns.NAMES:
            c, wc = cols[name], b.cols[name]
            assert c.shape == wc.shape and c.dtype == wc.dtype, (where, name)
            bad = np.nonzero((c != wc).reshape(len(c), -1).any(1))[0]
            assert len(bad) == 0, (where, name, f"{len(bad)} entries differ; first {bad[:5]}",
                                   c[bad[:3]], wc[bad[:3]])


# ---- CPU: the constructed cases and the sweep's expected columns -------------

@pytest.mark.parametrize("case", ["mostly_coded", "every_code", "window_edge"])
def test_constructed_cases_cpu(zp, golden, case):
    """Cases 6-8 are built, and their conditions hold, on the oracle alone."""
    assert get_case(zp, golden, case)


def test_window_sweep_columns_vs_getters(zp, golden):
    """On every descriptor of the window-edge sweep the oracle's columns equal
    the facade's getters: the expected columns of these shapes rest on two
    independent restatements of the reference's readers."""
    b = get_case(zp, golden, "window_edge")[0]
    firsts = {}
    for i, k in enumerate(b.frame_idx.tolist()):
        firsts.setdefault(k, i)
    getters = {k: getter_columns(zp, b.frames[k], b.want[i], b.wext[:, i])
               for k, i in firsts.items()}
    for i, k in enumerate(b.frame_idx.tolist()):
        # the same frame at another alignment: the same record and chains ...
        j = firsts[k]
        assert b.packed[i] == b.packed[j] and b.wext[:, i].tobytes() == b.wext[:, j].tobytes()
        for name, _, _ in orc.COLUMN_SPEC:             # ... and the getters' values
            assert np.array_equal(b.cols[name][i], getters[k][name]), (i, k, name)


# ---- GPU --------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("case", list(CASES))
def test_path_matches_oracle(zp, golden, slots, case, path):
    for b in get_case(zp, golden, case):
        for shift in b.shifts:
            got, gext, cols = run_path(zp, slots, path, b.arena, b.offs, b.lens, base_shift=shift)
            check(zp, b, path, shift, got, gext, cols)


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
def test_empty_batch(zp, slots, path):
    """n == 0 on every path: empty outputs, no error."""
    got, gext, cols = run_path(zp, slots, path, np.zeros(64, np.uint8), np.zeros(0, np.uint64),
                               np.zeros(0, np.uint32))
    assert len(got) == 0 and gext.shape == (2, 0)
    if path in ("fused", "split_codes"):
        assert sorted(cols) == sorted(zp.columns.NAMES)
        assert all(len(c) == 0 for c in cols.values())
    else:
        assert cols is None


def _c3_host(zp):
    a, o, l_ = zp.batch.generate_host("c3", 20000, first=21)
    want, wext = orc.parse_batch(a, o, l_)
    assert (want["err"] == 0).all()
    return a, o, l_, want, wext


@pytest.mark.gpu
def test_host_path_with_codes(zp, slots):
    """zp_parse_batch_host in 1 MiB chunks with record codes always: the
    expansion of a chunk lands before its copy back to the host."""
    a, o, l_, want, wext = _c3_host(zp)
    slots(1)
    lib = zp._lib.hip()
    ctx = lib.zp_ctx_create(0, 1 << 20)
    assert ctx
    rec = np.zeros(len(o), zp.records.RECORD_DTYPE)
    rec.view(np.uint8)[:] = 0xFF
    ext = np.zeros((2, len(o)), zp.records.EXT_DTYPE)
    rc = lib.zp_parse_batch_host(ctx, a.ctypes.data, len(a), o.ctypes.data, l_.ctypes.data,
                                 len(o), rec.ctypes.data, ext.ctypes.data)
    lib.zp_ctx_destroy(ctx)
    assert rc == 0, lib.zp_last_error()
    assert rec.tobytes() == orc.pack(want, wext).tobytes()
    assert zp.records.ext_match(ext, wext, want)


@pytest.mark.gpu
def test_ring_with_codes(zp, slots):
    """The host ring (3 slots of 1 MiB) with record codes always."""
    a, o, l_, want, wext = _c3_host(zp)
    slots(1)
    with zp.ring.Ring(0, 3, 1 << 20) as ring:
        got, gext = ring.parse(a, o, l_)
    assert got.tobytes() == orc.pack(want, wext).tobytes()
    assert zp.records.ext_match(gext, wext, want)
