"""Select and gather: filter parsed frames on the device
(zp_select_device, zp_gather_frames_device; semantics in include/zero_packet.h).

    sel = (select.Select(ok=True, has=("tcp",))
           .where("dest_port", eq=443).where("src_addr", prefix="10.0.0.0/8")
           .where("ip_version", eq=4))
    s = select.run(arena, offs, lens, records, sel, want=("idx", "packed_offs"))
    arena2, offs2, lens2, records2 = select.gather(arena, offs, lens, records, s)

A term's value is the entry columns.extract would give for that column (0 for
an error record or an absent reader, an IPv4 address in bytes 0-3 with zeros
behind), so a /8 over IPv4 also matches an IPv6 address that starts with the
same byte unless an ip_version term is added. Terms are ANDed.

The gathered tensors are a batch like any other: parse_batch, columns.extract
and columns.rewrite take them unchanged (pack=False: a view over the same
arena, so a rewrite through it edits the selected frames in place).
"""
import collections
import ctypes
import ipaddress

import numpy as np
import torch

from . import _lib, records as _rec
from .batch import check_batch
from .columns import COLUMNS, INDEX, width
from .records import EXT_BYTES, RECORD_BYTES

MAX_TERMS = 8                      # ZP_SELECT_MAX_TERMS
MASK_EQ, MASK_NE, RANGE, NOT_RANGE = 0, 1, 2, 3      # zp_sel_op
ERR_ANY, ERR_NONZERO = -1, -2      # ZP_SEL_ERR_*
SCAN_FRAMES = 262144               # ZP_SELECT_SCAN_FRAMES: one scan workgroup's frames

# zp_select_term / zp_select as numpy sees them (include/zero_packet.h)
TERM_DTYPE = np.dtype([("col", "u1"), ("op", "u1"), ("pad", "u1", (6,)), ("a", "u1", (16,)),
                       ("b", "u1", (16,))])
SELECT_DTYPE = np.dtype([("flags_all", "<u4"), ("flags_any", "<u4"), ("flags_none", "<u4"),
                         ("err", "<i4"), ("min_len", "<u4"), ("max_len", "<u4"),
                         ("nterms", "<u4"), ("terms", TERM_DTYPE, (MAX_TERMS,))])
assert TERM_DTYPE.itemsize == 40 and SELECT_DTYPE.itemsize == 28 + 40 * MAX_TERMS

# reader names of has= / lacks= / any_of= -> record flag bits (records.F_*)
READERS = {"ethernet": _rec.F_ETHERNET, "arp": _rec.F_ARP, "ipv4": _rec.F_IPV4,
           "ipv6": _rec.F_IPV6, "ip_in_ip": _rec.F_IP_IN_IP, "ip_in_ip_v6": _rec.F_IP_IN_IP_V6,
           "tcp": _rec.F_TCP, "udp": _rec.F_UDP, "icmpv4": _rec.F_ICMPV4,
           "icmpv6": _rec.F_ICMPV6, "ext": _rec.F_EXT, "inner_ext": _rec.F_INNER_EXT}

Selection = collections.namedtuple("Selection", "count idx packed_offs mask")


def _flags(names):
    if isinstance(names, int):
        return names & _rec.F_MASK
    if isinstance(names, str):
        names = (names,)
    f = 0
    for name in names:
        if name not in READERS:
            raise ValueError(f"unknown reader {name!r} (select.READERS)")
        f |= READERS[name]
    return f


def _operand(name, v):
    """A term operand in the column's layout: width bytes (LE scalar or the
    byte array as extracted)."""
    _, dt, k = COLUMNS[INDEX[name]]
    w = width(name)
    if k > 1:
        b = bytes(v)
        if len(b) != w:
            raise ValueError(f"column {name!r}: operand must have {w} bytes, not {len(b)}")
        return b
    if isinstance(v, (bytes, bytearray)):
        raise ValueError(f"column {name!r} is a scalar column: operand must be an integer")
    v = int(v)
    if not 0 <= v < 1 << (8 * w):
        raise ValueError(f"column {name!r}: operand {v} does not fit {w} bytes")
    return v.to_bytes(w, "little")


class Select:
    """A selector: the record predicate, the length bounds and up to
    MAX_TERMS column terms, all ANDed.

    ok=True: accepted frames (err == 0); ok=False: rejected ones. err: a
    records.ERR name or code (exactly that error). has / lacks / any_of:
    reader names (select.READERS) or a raw flag mask: all present / none
    present / at least one present. min_len / max_len: inclusive bounds on the
    frame length."""

    def __init__(self, ok=None, has=(), lacks=(), any_of=(), err=None, min_len=0,
                 max_len=0xFFFFFFFF):
        if ok is not None and err is not None:
            raise ValueError("give ok= or err=, not both")
        if err is None:
            self.err = ERR_ANY if ok is None else (0 if ok else ERR_NONZERO)
        elif isinstance(err, str):
            if err not in _rec.ERR:
                raise ValueError(f"unknown error name {err!r} (records.ERR_NAMES)")
            self.err = _rec.ERR[err]
        else:
            self.err = int(err)
        self.flags_all, self.flags_none, self.flags_any = _flags(has), _flags(lacks), _flags(any_of)
        if not (0 <= int(min_len) <= 0xFFFFFFFF and 0 <= int(max_len) <= 0xFFFFFFFF):
            raise ValueError("length bounds must fit 32 bits")
        self.min_len, self.max_len = int(min_len), int(max_len)
        self.terms = []            # (column name, op, a bytes, b bytes)

    def where(self, name, eq=None, ne=None, mask=None, between=None, outside=None, prefix=None,
              mac=None):
        """Adds one term on column `name` and returns self.
        eq / ne: the value (with mask=: (v & mask) == eq / != ne); between /
        outside=(lo, hi): inclusive unsigned range, scalar columns only;
        prefix="10.0.0.0/8" | "2001:db8::/32": address columns; mac=
        "aa:bb:cc:dd:ee:ff" or 6 bytes: MAC columns."""
        if name not in INDEX:
            raise ValueError(f"unknown column {name!r}")
        if sum(x is not None for x in (eq, ne, between, outside, prefix, mac)) != 1:
            raise ValueError("give exactly one of eq, ne, between, outside, prefix, mac")
        if len(self.terms) >= MAX_TERMS:
            raise ValueError(f"at most {MAX_TERMS} terms")
        _, dt, k = COLUMNS[INDEX[name]]
        w = width(name)
        if between is not None or outside is not None:
            if k > 1:
                raise ValueError(f"column {name!r} is a byte array: no range terms")
            if mask is not None:
                raise ValueError("mask= goes with eq / ne")
            lo, hi = between if between is not None else outside
            term = (name, RANGE if between is not None else NOT_RANGE, _operand(name, lo),
                    _operand(name, hi))
        elif prefix is not None:
            if w != 16:
                raise ValueError(f"column {name!r} is not an address column")
            net = ipaddress.ip_network(prefix, strict=False)
            pad = 16 - len(net.network_address.packed)
            term = (name, MASK_EQ, net.network_address.packed + bytes(pad),
                    net.netmask.packed + bytes(pad))
        elif mac is not None:
            if w != 6:
                raise ValueError(f"column {name!r} is not a MAC column")
            b = bytes.fromhex(mac.replace(":", "").replace("-", "")) if isinstance(mac, str) \
                else bytes(mac)
            term = (name, MASK_EQ, _operand(name, b), b"\xff" * 6)
        else:
            v = eq if eq is not None else ne
            m = _operand(name, mask) if mask is not None else b"\xff" * w
            term = (name, MASK_EQ if eq is not None else MASK_NE, _operand(name, v), m)
        self.terms.append(term)
        return self

    def encode(self):
        """The zp_select struct as a one-element numpy array (SELECT_DTYPE)."""
        s = np.zeros(1, SELECT_DTYPE)
        s["flags_all"], s["flags_any"], s["flags_none"] = self.flags_all, self.flags_any, \
            self.flags_none
        s["err"], s["min_len"], s["max_len"] = self.err, self.min_len, self.max_len
        s["nterms"] = len(self.terms)
        for k, (name, op, a, b) in enumerate(self.terms):
            t = s["terms"][0][k]
            t["col"], t["op"] = INDEX[name], op
            t["a"][:len(a)] = np.frombuffer(a, np.uint8)
            t["b"][:len(b)] = np.frombuffer(b, np.uint8)
        return s


def _stream(stream, device):
    return ctypes.c_void_p(stream) if stream is not None else \
        ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _ptr(t):
    return t.data_ptr() if t is not None else None


def run(arena, offs, lens, records, sel, want=("idx",), out=None, stream=None, check=True):
    """Evaluates `sel` over a parsed batch; returns Selection(count, idx,
    packed_offs, mask) of device tensors (those not in `want` are None).
    count: int64 [2] = {selected frames, their bytes}; idx: int32 [n], the
    selected indices in [0, count[0]), ascending; packed_offs: int64 [n], the
    back-to-back offsets of the selected frames; mask: int64 [ceil(n / 64)],
    bit i % 64 of word i / 64. Entries of idx / packed_offs at and past
    count[0] are not written. `out` may hold preallocated tensors under the
    same names (and "scratch", uint8). Without terms arena / offs may be
    None. check: as in batch.parse_batch (the descriptor bounds reduction,
    which synchronises); check=False makes the call enqueue-only: run itself
    never reads a result back."""
    if not isinstance(sel, Select):
        raise TypeError("sel must be a select.Select")
    bad = set(want) - {"idx", "packed_offs", "mask"}
    if bad:
        raise ValueError(f"unknown outputs {sorted(bad)}")
    for t in (arena, offs, lens, records):
        if t is not None and not t.is_cuda:
            raise RuntimeError("select.run needs device tensors (no CPU fallback)")
    if sel.terms and (arena is None or offs is None or lens is None):
        raise ValueError("a selector with terms needs arena, offs and lens")
    dev = records.device
    n = records.numel() * records.element_size() // RECORD_BYTES
    if arena is not None and offs is not None and lens is not None:
        check_batch(arena, offs, lens, ((records, RECORD_BYTES),), bounds=check and bool(sel.terms),
                    stream=stream)
    elif not records.is_contiguous():
        raise ValueError("records must be contiguous")
    if lens is not None and (lens.dtype != torch.int32 or lens.numel() != n or
                             not lens.is_contiguous()):
        raise ValueError(f"lens must be contiguous int32 with {n} entries")
    out = dict(out or {})
    lib = _lib.hip()

    def buf(name, shape, dtype):
        t = out.get(name)
        if t is None:
            return torch.empty(shape, dtype=dtype, device=dev)
        if t.dtype != dtype or t.device != dev or not t.is_contiguous() or \
                t.numel() < int(np.prod(shape)):
            raise ValueError(f"out[{name!r}] must be a contiguous {dtype} tensor on {dev} with "
                             f"at least {int(np.prod(shape))} elements")
        return t
    count = buf("count", (2,), torch.int64)
    idx = buf("idx", (n,), torch.int32) if "idx" in want else None
    packed = buf("packed_offs", (n,), torch.int64) if "packed_offs" in want else None
    mask = buf("mask", ((n + 63) // 64,), torch.int64) if "mask" in want else None
    nscratch = int(lib.zp_select_scratch_bytes(n))
    scratch = buf("scratch", (nscratch,), torch.uint8)
    enc = sel.encode()
    rc = lib.zp_select_device(_ptr(arena), _ptr(offs), _ptr(lens), records.data_ptr(), n,
                              enc.ctypes.data, _ptr(mask), _ptr(idx), _ptr(packed),
                              count.data_ptr(), scratch.data_ptr(),
                              scratch.numel(), _stream(stream, dev))
    _lib.check(rc, "zp_select_device")
    if stream is not None:                    # the allocator must not hand scratch on early
        scratch.record_stream(torch.cuda.ExternalStream(int(stream), device=dev))
    return Selection(count, idx, packed, mask)


def gather(arena, offs, lens, records, selection, ext=None, pack=True, capacity=None, out=None,
           stream=None):
    """The selected frames as a batch of their own: (arena2, offs2, lens2,
    records2), and ext2 behind them when `ext` is given.
    pack=True copies the frames back to back into a fresh arena (selection
    must hold packed_offs); pack=False returns a view: arena2 is `arena` and
    offs2 point into it. Without `capacity` / `out` the call reads
    selection.count back to size its outputs exactly: that is ONE
    SYNCHRONISATION with the device. With capacity=(frames, bytes) (or an int:
    frames, and the arena's size for the bytes) or out={"arena", "offs",
    "lens", "records", "ext"} the outputs have that fixed size, only their
    first count[0] entries (count[1] bytes) are written and the call is
    enqueue-only, so it captures into a graph; the consumer takes the valid
    length from selection.count."""
    for t in (arena, offs, lens, records):
        if not t.is_cuda:
            raise RuntimeError("select.gather needs device tensors (no CPU fallback)")
    if selection.idx is None:
        raise ValueError("selection has no idx (run(..., want=('idx', ...)))")
    if pack and selection.packed_offs is None:
        raise ValueError("pack=True needs packed_offs (run(..., want=('idx', 'packed_offs')))")
    check_batch(arena, offs, lens, ((records, RECORD_BYTES), (ext, 2 * EXT_BYTES)), bounds=False)
    dev = arena.device
    n = offs.numel()
    out = dict(out or {})
    if capacity is None and not out:
        m, nbytes = (int(v) for v in selection.count.tolist())       # the one synchronisation
    elif capacity is not None:
        m, nbytes = capacity if isinstance(capacity, (tuple, list)) else (capacity, arena.numel())
    else:
        m = out["offs"].numel()
        nbytes = out["arena"].numel() if pack else 0
    m = min(int(m), n)

    def buf(name, shape, dtype):
        t = out.get(name)
        if t is None:
            return torch.empty(shape, dtype=dtype, device=dev)
        if t.dtype != dtype or t.device != dev or not t.is_contiguous() or \
                t.numel() != int(np.prod(shape)):
            raise ValueError(f"out[{name!r}] must be a contiguous {dtype} tensor on {dev} of "
                             f"shape {tuple(shape)}")
        return t
    offs2 = buf("offs", (m,), torch.int64)
    lens2 = buf("lens", (m,), torch.int32)
    recs2 = buf("records", (m, RECORD_BYTES), torch.uint8)
    ext2 = buf("ext", (2, m, EXT_BYTES), torch.uint8) if ext is not None else None
    arena2 = buf("arena", (int(nbytes),), torch.uint8) if pack else arena
    rc = _lib.hip().zp_gather_frames_device(
        arena.data_ptr(), offs.data_ptr(), lens.data_ptr(), records.data_ptr(), _ptr(ext), n,
        selection.idx.data_ptr(), _ptr(selection.packed_offs) if pack else None, m,
        selection.count.data_ptr(), arena2.data_ptr() if pack else None,
        arena2.numel() if pack else 0, offs2.data_ptr(), lens2.data_ptr(), recs2.data_ptr(),
        _ptr(ext2), _stream(stream, dev))
    _lib.check(rc, "zp_gather_frames_device")
    return (arena2, offs2, lens2, recs2) + ((ext2,) if ext is not None else ())
