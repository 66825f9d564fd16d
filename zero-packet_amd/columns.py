"""Column views over parsed frames (zp_extract_columns_device).

    cols = columns.extract(arena, offs, lens, records, names=("src_port", ...))

Each column is a device tensor of n entries (byte-array columns: [n, width]
uint8): the reader getters of every frame gathered into SoA form, so a
downstream consumer (flow table, filter, sampler) needs no host pass. Column
semantics and the reference getters they follow: include/zero_packet.h
(zp_col). Entry i is 0 when record i holds an error or the reader is absent.
"""
import collections
import ctypes

import numpy as np
import torch

from . import _lib
from .batch import alloc_outputs, check_batch
from .records import EXT_BYTES, RECORD_BYTES

# (name, torch dtype, elements per frame) in zp_col order.
COLUMNS = [
    ("dest_mac", torch.uint8, 6), ("src_mac", torch.uint8, 6),
    ("ethertype", torch.uint16, 1), ("vlan_tci", torch.uint16, 1),
    ("vlan_inner_tci", torch.uint16, 1), ("arp_oper", torch.uint16, 1),
    ("ip_version", torch.uint8, 1), ("src_addr", torch.uint8, 16),
    ("dest_addr", torch.uint8, 16), ("protocol", torch.uint8, 1), ("ttl", torch.uint8, 1),
    ("tos", torch.uint8, 1), ("ip_id", torch.uint32, 1), ("ip_len", torch.uint16, 1),
    ("inner_version", torch.uint8, 1), ("inner_src_addr", torch.uint8, 16),
    ("inner_dest_addr", torch.uint8, 16), ("inner_protocol", torch.uint8, 1),
    ("l4_proto", torch.uint8, 1), ("src_port", torch.uint16, 1), ("dest_port", torch.uint16, 1),
    ("tcp_seq", torch.uint32, 1), ("tcp_ack", torch.uint32, 1), ("tcp_flags", torch.uint8, 1),
    ("tcp_window", torch.uint16, 1), ("icmp_type", torch.uint8, 1),
    ("icmp_code", torch.uint8, 1), ("l4_checksum", torch.uint16, 1),
    ("payload_off", torch.uint32, 1),
]
NAMES = [c[0] for c in COLUMNS]
INDEX = {name: k for k, name in enumerate(NAMES)}
NUMPY_DTYPE = {torch.uint8: np.uint8, torch.uint16: np.uint16, torch.uint32: np.uint32}


def width(name):
    _, dt, k = COLUMNS[INDEX[name]]
    return k * torch.empty((), dtype=dt).element_size()


def _alloc(name, n, device):
    _, dt, k = COLUMNS[INDEX[name]]
    return torch.empty((n, k) if k > 1 else (n,), dtype=dt, device=device)


def extract(arena, offs, lens, records, names=None, out=None, stream=None, check=True):
    """Fills the requested columns (default: all) on the device; returns
    {name: tensor}. `out` may hold preallocated tensors. check: as in
    batch.parse_batch (descriptor bounds reduction)."""
    for t in (arena, offs, lens, records):
        if not t.is_cuda:
            raise RuntimeError("columns.extract needs device tensors (no CPU fallback)")
    n = offs.numel()
    check_batch(arena, offs, lens, ((records, RECORD_BYTES),), bounds=check)
    names = list(names) if names is not None else NAMES
    out = dict(out or {})
    ptrs = (ctypes.c_void_p * len(COLUMNS))()
    for name in names:
        if name not in out:
            out[name] = _alloc(name, n, arena.device)
        t = out[name]
        assert t.is_contiguous() and t.numel() * t.element_size() == n * width(name), name
        ptrs[INDEX[name]] = t.data_ptr()
    s = ctypes.c_void_p(stream) if stream is not None else \
        ctypes.c_void_p(torch.cuda.current_stream(arena.device).cuda_stream)
    rc = _lib.hip().zp_extract_columns_device(arena.data_ptr(), offs.data_ptr(), lens.data_ptr(),
                                              records.data_ptr(), n, ptrs, s)
    _lib.check(rc, "zp_extract_columns_device")
    return {k: out[k] for k in names}


# The columns zp_rewrite_columns_device writes back (zp_col_writable).
WRITABLE = ("dest_mac", "src_mac", "vlan_tci", "vlan_inner_tci", "src_addr", "dest_addr", "ttl",
            "tos", "ip_id", "src_port", "dest_port", "tcp_seq", "tcp_ack", "tcp_window")


def rewrite(arena, offs, lens, records, cols, stream=None, check=True):
    """Writes columns back into the parsed frames, in place, and refreshes the
    IPv4 header and L4 checksums (zp_rewrite_columns_device; semantics in
    include/zero_packet.h). cols: {name: device tensor} of WRITABLE columns in
    the layout extract() returns; fields of columns not given stay. records
    are the ones the parse wrote for this batch; they stay valid afterwards.
    check=True validates the descriptors and that no two frames overlap, as
    BuildBatch.run does (one device sort and reduction, then a sync)."""
    from .builder import check_disjoint
    for t in (arena, offs, lens, records):
        if not t.is_cuda:
            raise RuntimeError("columns.rewrite needs device tensors (no CPU fallback)")
    n = offs.numel()
    ptrs = (ctypes.c_void_p * len(COLUMNS))()
    for name, t in cols.items():
        if name not in INDEX:
            raise ValueError(f"unknown column {name!r}")
        if name not in WRITABLE:
            raise ValueError(f"column {name!r} is not writable (columns.WRITABLE)")
        _, dt, k = COLUMNS[INDEX[name]]
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != arena.device:
            raise ValueError(f"column {name!r} must be a tensor on {arena.device}")
        if t.dtype != dt:
            raise ValueError(f"column {name!r} must be {dt}, not {t.dtype}")
        if not t.is_contiguous() or t.numel() != n * k or \
                t.numel() * t.element_size() != n * width(name):
            raise ValueError(f"column {name!r} must be contiguous with {n} x {k} elements")
        ptrs[INDEX[name]] = t.data_ptr()
    check_batch(arena, offs, lens, ((records, RECORD_BYTES),), bounds=check, stream=stream)
    if check:
        check_disjoint(offs, lens, stream)
    s = ctypes.c_void_p(stream) if stream is not None else \
        ctypes.c_void_p(torch.cuda.current_stream(arena.device).cuda_stream)
    rc = _lib.hip().zp_rewrite_columns_device(arena.data_ptr(), offs.data_ptr(), lens.data_ptr(),
                                              records.data_ptr(), n, ptrs, s)
    _lib.check(rc, "zp_rewrite_columns_device")


# Path choice of parse_with_columns(mode="auto") per workload: the fused
# kernel (one pass) wins on most traffic, but plain IPv4 frames with wide
# column requests run faster as parse + extract (round 4/5: c3 with all 29
# columns +2-5 % fused; c4/c5/c6 -11 to -23 %).
#
# A workload is its shape (device, column set, batch-size octave) and the
# traffic's stack mix: shares of plain IPv4, of IPv6 extension chains and of
# IP-in-IP among 256 records sampled from a call of that shape (copied back
# asynchronously and read on a later call once its event has completed, every
# _SAMPLE_EVERY calls per shape, so a reused arena whose traffic changes is
# re-classified). An undecided workload alternates the two paths, one per
# call, each between two timing events; once both have _AUTO_REPS completed
# timings, the faster is kept. Nothing here waits for the device: events are
# only queried, and every call runs exactly one path.
_AUTO_REPS = 2             # completed timings per path before a choice
_AUTO_MAX = 256            # workloads remembered (least recently used dropped)
_SAMPLE = 256              # records sampled per mix reading
_SAMPLE_EVERY = 16         # calls per shape between two mix readings
_auto = collections.OrderedDict()   # workload key -> "fused" | "split"
_timing = {}               # undecided workload key -> {"fused": [...], "split": [...], "pending": [...]}
_shapes = {}               # shape -> _ShapeState
auto_timings = 0           # timed runs started (diagnostics, tests)


class _ShapeState:
    def __init__(self):
        self.mix = None            # current stack-mix class (None: not read yet)
        self.calls = 0
        self.pending = None        # (pinned sample, event) of a mix reading in flight
        self.host = None           # pinned sample buffer
        self.idx = None            # device sample indices (for self.n)
        self.n = -1


def _shape_key(arena, n, names):
    return (arena.device.index, tuple(sorted(names)), max(n, 1).bit_length())


def _mix_class(sample):
    """Stack-mix class of sampled records (uint8 [k, 8]): quarters of the
    plain-IPv4, extension-chain and IP-in-IP shares among accepted frames."""
    from .records import F_EXT, F_INNER_EXT, F_IP_IN_IP, F_IPV4
    w = sample.numpy().view(np.uint32).reshape(-1, 2)
    flags, offs = w[:, 0], w[:, 1]
    ok = (flags >> 26) == 0
    k = max(int(ok.sum()), 1)
    v4 = ok & ((flags & F_IPV4) != 0) & ((flags & F_IP_IN_IP) == 0)
    chain = ok & (((flags & (F_EXT | F_INNER_EXT)) != 0) | ((offs >> 31) != 0))
    inner = ok & ((flags & F_IP_IN_IP) != 0)
    q = lambda m: int(round(4 * int(m.sum()) / k))
    return (q(v4), q(chain), q(inner))


def reset_auto():
    """Forgets every choice and mix reading of parse_with_columns(mode="auto")."""
    _auto.clear()
    _timing.clear()
    _shapes.clear()


def _remember(key, choice):
    _auto[key] = choice
    _auto.move_to_end(key)
    while len(_auto) > _AUTO_MAX:
        _auto.popitem(last=False)


def auto_choice(arena, n, names):
    """The path parse_with_columns(mode="auto") uses for this shape and the
    traffic mix read last (None while undecided)."""
    sk = _shape_key(arena, n, names)
    st = _shapes.get(sk)
    return _auto.get(sk + ((st.mix if st else None),))


def _read_mix(st):
    if st.pending is not None and st.pending[1].query():
        st.mix = _mix_class(st.pending[0])
        st.pending = None


def _sample_mix(st, records, n, ts):
    """Queues a copy of _SAMPLE records (evenly spaced) to pinned memory."""
    k = min(_SAMPLE, n)
    if st.n != n:
        st.idx = torch.linspace(0, n - 1, k, device=records.device).round().long()
        st.host = torch.empty((k, 8), dtype=torch.uint8, pin_memory=True)
        st.n = n
    with torch.cuda.stream(ts):
        st.host.copy_(records.index_select(0, st.idx), non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(ts)
    st.pending = (st.host, ev)


def _collect(t):
    """Moves the completed timings of an undecided workload into its lists."""
    left = []
    for path, a, b in t["pending"]:
        if b.query():
            t[path].append(a.elapsed_time(b))
        else:
            left.append((path, a, b))
    t["pending"] = left


def parse_with_columns(arena, offs, lens, names=None, records=None, ext=None, out=None,
                       stream=None, check=True, mode="auto"):
    """Records and the requested columns of every frame. Returns (records,
    ext, {name: tensor}); the results are the same on every path.
    mode: "fused" = zp_parse_batch_columns_device (one pass over the frames);
    "split" = zp_parse_batch_device then zp_extract_columns_device on the same
    stream; "auto" (default) = the faster of the two for this workload (device,
    column set, batch-size octave and the stack mix of the traffic, read from
    sampled records; reset_auto() forgets the choices). Every call runs one
    path and returns without waiting for the device: while a workload is
    undecided its calls alternate the paths between timing events, and the
    first call after both paths have two completed timings fixes the choice.
    Under stream capture "auto" runs the known choice (or the fused path)
    with no events and no sampling."""
    for t in (arena, offs, lens):
        if not t.is_cuda:
            raise RuntimeError("columns.parse_with_columns needs device tensors (no CPU fallback)")
    if mode not in ("auto", "fused", "split"):
        raise ValueError(f"mode {mode!r}: auto, fused or split")
    n = offs.numel()
    d = arena.device
    records, ext = alloc_outputs(n, d, records, ext)
    names = list(names) if names is not None else NAMES
    out = dict(out or {})
    ptrs = (ctypes.c_void_p * len(COLUMNS))()
    for name in names:
        if name not in out:
            out[name] = _alloc(name, n, d)
        ptrs[INDEX[name]] = out[name].data_ptr()
    check_batch(arena, offs, lens, [(records, RECORD_BYTES), (ext, 2 * EXT_BYTES)] +
                [(out[k], width(k)) for k in names], bounds=check)
    s = ctypes.c_void_p(stream) if stream is not None else \
        ctypes.c_void_p(torch.cuda.current_stream(d).cuda_stream)
    lib = _lib.hip()

    def fused():
        _lib.check(lib.zp_parse_batch_columns_device(arena.data_ptr(), offs.data_ptr(),
                                                     lens.data_ptr(), n, records.data_ptr(),
                                                     ext.data_ptr(), ptrs, s),
                   "zp_parse_batch_columns_device")

    def split():
        _lib.check(lib.zp_parse_batch_device(arena.data_ptr(), offs.data_ptr(), lens.data_ptr(),
                                             n, records.data_ptr(), ext.data_ptr(), s),
                   "zp_parse_batch_device")
        _lib.check(lib.zp_extract_columns_device(arena.data_ptr(), offs.data_ptr(),
                                                 lens.data_ptr(), records.data_ptr(), n, ptrs, s),
                   "zp_extract_columns_device")
    paths = {"fused": fused, "split": split}
    if mode != "auto" or n == 0:
        paths[mode if mode != "auto" else "fused"]()
        return records, ext, {k: out[k] for k in names}
    if torch.cuda.is_current_stream_capturing():
        # under graph capture: no timing events, no mix readings
        sk = _shape_key(arena, n, names)
        st = _shapes.get(sk)
        paths[_auto.get(sk + ((st.mix if st else None),)) or "fused"]()
        return records, ext, {k: out[k] for k in names}
    ts = torch.cuda.ExternalStream(stream, device=d) if stream is not None else \
        torch.cuda.current_stream(d)
    sk = _shape_key(arena, n, names)
    st = _shapes.get(sk)
    if st is None:
        st = _shapes[sk] = _ShapeState()
        while len(_shapes) > _AUTO_MAX:
            del _shapes[next(iter(_shapes))]
    _read_mix(st)
    key = sk + (st.mix,)
    choice = _auto.get(key)
    if choice is not None:
        _auto.move_to_end(key)
        paths[choice]()
    else:
        t = _timing.setdefault(key, {"fused": [], "split": [], "pending": []})
        _collect(t)
        if len(t["fused"]) >= _AUTO_REPS and len(t["split"]) >= _AUTO_REPS:
            choice = min(("fused", "split"), key=lambda p: min(t[p]))
            _remember(key, choice)
            del _timing[key]
            paths[choice]()
        else:
            # time the path with fewer timings (counting those in flight)
            nf = len(t["fused"]) + sum(1 for p, _, _ in t["pending"] if p == "fused")
            ns = len(t["split"]) + sum(1 for p, _, _ in t["pending"] if p == "split")
            path = "fused" if nf <= ns else "split"
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(ts)
            paths[path]()
            b.record(ts)
            t["pending"].append((path, a, b))
            global auto_timings
            auto_timings += 1
            if len(_timing) > _AUTO_MAX:
                del _timing[next(iter(_timing))]
    if st.pending is None and (st.mix is None or st.calls % _SAMPLE_EVERY == 0):
        _sample_mix(st, records, n, ts)
    st.calls += 1
    return records, ext, {k: out[k] for k in names}
