"""Flow table: group parsed frames by key on the device, with per-flow counters
(zp_flow_aggregate_device; semantics in include/zero_packet.h).

    t = flows.aggregate(arena, offs, lens, records)            # the 5-tuple
    t.flow_of            # int32 [n]: frame i's flow number, -1 (FLOW_NONE) if not keyed
    t.count              # int64 [4]: {F, keyed frames, keyed bytes, overflow}
    entries = flows.to_numpy(t)                                 # FLOW_DTYPE [F]: synchronises

A frame is keyed when it parsed without error and has an outer IPv4 / IPv6
reader (and its bit of `mask` is set, when one is given). The key holds the
outer addresses and ip_version always; ports=, proto=, vlan= add the L4 ports,
l4_proto and the VLAN id; bidir=True makes both directions one flow. Flows are
numbered in ascending order of their first frame, so every output is the same
from run to run.

flows.Table keeps the same grouping across batches (zp_flow_update_device,
zp_flow_retire_device): see the class.
"""
import collections
import ctypes

import numpy as np
import torch

from . import _lib
from .batch import check_batch
from .records import RECORD_BYTES

PORTS, PROTO, VLAN, BIDIR = 1, 2, 4, 8         # ZP_FLOW_*
FLOW_NONE = 0xFFFFFFFF                         # ZP_FLOW_NONE (-1 in the int32 flow_of tensor)

# zp_flow_key / zp_flow_entry / zp_flow_opts as numpy sees them (include/zero_packet.h)
KEY_DTYPE = np.dtype([("src_addr", "u1", (16,)), ("dest_addr", "u1", (16,)), ("src_port", "<u2"),
                      ("dest_port", "<u2"), ("l4_proto", "u1"), ("ip_version", "u1"),
                      ("vlan", "<u2")])
FLOW_DTYPE = np.dtype([("key", KEY_DTYPE), ("first", "<u4"), ("last", "<u4"), ("packets", "<u4"),
                       ("tcp_flags", "u1"), ("pad", "u1", (3,)), ("bytes", "<u8")])
OPTS_DTYPE = np.dtype([("key_flags", "<u4"), ("pad", "<u4"), ("max_flows", "<u8"),
                       ("hash_mask", "<u8")])
assert KEY_DTYPE.itemsize == 40 and FLOW_DTYPE.itemsize == 64 and OPTS_DTYPE.itemsize == 24

FlowTable = collections.namedtuple("FlowTable", "count flows flow_of")


def key_flags(ports=True, proto=True, vlan=False, bidir=False):
    return (PORTS if ports else 0) | (PROTO if proto else 0) | (VLAN if vlan else 0) | \
        (BIDIR if bidir else 0)


def encode_opts(flags, max_flows, hash_mask=None):
    """The zp_flow_opts struct as a one-element numpy array (OPTS_DTYPE)."""
    flags, max_flows = int(flags), int(max_flows)
    if flags & ~(PORTS | PROTO | VLAN | BIDIR) or flags < 0:
        raise ValueError(f"unknown key flags {flags:#x}")
    if not 0 < max_flows < 1 << 64:
        raise ValueError("max_flows must be positive")
    hash_mask = 0xFFFFFFFFFFFFFFFF if hash_mask is None else int(hash_mask)
    if not 0 <= hash_mask < 1 << 64:
        raise ValueError("hash_mask must fit 64 bits")
    o = np.zeros(1, OPTS_DTYPE)
    o["key_flags"], o["max_flows"], o["hash_mask"] = flags, max_flows, hash_mask
    return o


def _stream(stream, device):
    return ctypes.c_void_p(stream) if stream is not None else \
        ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def aggregate(arena, offs, lens, records, ports=True, proto=True, vlan=False, bidir=False,
              max_flows=None, mask=None, want=("flow_of",), out=None, stream=None, check=True,
              hash_mask=None):
    """Groups the keyed frames of a parsed batch; returns FlowTable(count,
    flows, flow_of) of device tensors. count: int64 [4] = {F, keyed frames,
    keyed bytes, overflow}; flows: uint8 [max_flows, 64], zp_flow_entry
    (FLOW_DTYPE) rows of which the first F are written; flow_of: int32 [n]
    (None unless in `want`). max_flows=None means n (it can then not
    overflow). mask: the int64 words select.run(want=("mask",)) gives: only
    frames whose bit is set are keyed. `out` may hold preallocated tensors
    under "count", "flows", "flow_of" and "scratch" (uint8). check: as in
    batch.parse_batch (the descriptor bounds reduction, which synchronises);
    check=False makes the call enqueue-only, so it captures into a graph.
    hash_mask is ANDed into the key's hash: tests pass small values to force
    collisions; the results do not depend on it."""
    bad = set(want) - {"flow_of"}
    if bad:
        raise ValueError(f"unknown outputs {sorted(bad)}")
    for t in (arena, offs, lens, records, mask):
        if t is not None and not t.is_cuda:
            raise RuntimeError("flows.aggregate needs device tensors (no CPU fallback)")
    check_batch(arena, offs, lens, ((records, RECORD_BYTES),), bounds=check, stream=stream)
    dev = arena.device
    n = offs.numel()
    if max_flows is None:
        max_flows = max(n, 1)
    enc = encode_opts(key_flags(ports, proto, vlan, bidir), max_flows, hash_mask)
    max_flows = int(max_flows)
    if mask is not None and (mask.dtype != torch.int64 or mask.device != dev or
                             not mask.is_contiguous() or mask.numel() < (n + 63) // 64):
        raise ValueError(f"mask must be a contiguous int64 tensor on {dev} with at least "
                         f"{(n + 63) // 64} words")
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
    count = buf("count", (4,), torch.int64)
    table = buf("flows", (max_flows, FLOW_DTYPE.itemsize), torch.uint8)
    flow_of = buf("flow_of", (n,), torch.int32) if "flow_of" in want else None
    scratch = buf("scratch", (int(lib.zp_flow_scratch_bytes(n, max_flows)),), torch.uint8)
    rc = lib.zp_flow_aggregate_device(
        arena.data_ptr(), offs.data_ptr(), lens.data_ptr(), records.data_ptr(), n, enc.ctypes.data,
        mask.data_ptr() if mask is not None else None,
        flow_of.data_ptr() if flow_of is not None else None, table.data_ptr(), count.data_ptr(),
        scratch.data_ptr(), scratch.numel(), _stream(stream, dev))
    _lib.check(rc, "zp_flow_aggregate_device")
    if stream is not None:                    # the allocator must not hand scratch on early
        scratch.record_stream(torch.cuda.ExternalStream(int(stream), device=dev))
    return FlowTable(count, table, flow_of)


def to_numpy(table):
    """The first F entries as a FLOW_DTYPE array. Reads table.count back:
    that is ONE SYNCHRONISATION with the device. Raises on overflow (F above
    the table's capacity: only count[3] is defined then)."""
    f, _, _, overflow = (int(v) for v in table.count.tolist())     # the one synchronisation
    if overflow:
        raise RuntimeError("flow table overflow: more flows than max_flows")
    rows = table.flows.view(-1, FLOW_DTYPE.itemsize)[:f]
    return rows.cpu().numpy().reshape(-1).view(FLOW_DTYPE).copy()


# ---- the persistent table ----------------------------------------------------

IDLE_NEVER = 0xFFFFFFFF                        # ZP_FLOW_IDLE_NEVER
# zp_flow_state as numpy sees it (include/zero_packet.h)
STATE_DTYPE = np.dtype([("key", KEY_DTYPE), ("first_epoch", "<u4"), ("last_epoch", "<u4"),
                        ("packets_flags", "<u8"), ("bytes", "<u8")])
assert STATE_DTYPE.itemsize == 64
TABLE_HEADER_BYTES = 64                        # {magic, signature, F, epoch, 4 spare words}

TableUpdate = collections.namedtuple("TableUpdate", "count flow_of")
TableRetire = collections.namedtuple("TableRetire", "count retired remap")


def state_packets(entries):
    """ZP_FLOW_STATE_PACKETS over a STATE_DTYPE array."""
    return entries["packets_flags"] & np.uint64(0x00FFFFFFFFFFFFFF)


def state_tcp_flags(entries):
    """ZP_FLOW_STATE_TCP_FLAGS over a STATE_DTYPE array."""
    return (entries["packets_flags"] >> np.uint64(56)).astype(np.uint8)


def _buf(out, name, shape, dtype, dev):
    t = out.get(name)
    if t is None:
        return torch.empty(shape, dtype=dtype, device=dev)
    if t.dtype != dtype or t.device != dev or not t.is_contiguous() or t.numel() < int(np.prod(shape)):
        raise ValueError(f"out[{name!r}] must be a contiguous {dtype} tensor on {dev} with at least "
                         f"{int(np.prod(shape))} elements")
    return t


class Table:
    """A flow table that persists across batches (zp_flow_table_init_device,
    zp_flow_update_device, zp_flow_retire_device; the rule is in
    include/zero_packet.h). It owns its device tensors: `table` (uint8: the
    header and the hash slots) and `flows` (uint8 [max_flows, 64],
    zp_flow_state / STATE_DTYPE rows of which the first F are live).

        t = flows.Table(1 << 20, "cuda:0")                 # the 5-tuple
        u = t.update(arena, offs, lens, records)           # u.count int64 [8], u.flow_of int32 [n]
        r = t.retire(max_idle=8, tcp_any=0x05)             # r.count int64 [2], r.retired, r.remap
        entries = t.to_numpy()                             # STATE_DTYPE [F]: synchronises

    The options are fixed here. Flows keep their numbers from update to
    update; a retire compacts them in order and says so in `remap`. `out` may
    hold preallocated "table" and "flows" tensors (uint8)."""

    def __init__(self, max_flows, device, ports=True, proto=True, vlan=False, bidir=False,
                 hash_mask=None, out=None, stream=None):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("flows.Table needs a device (no CPU fallback)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.max_flows = int(max_flows)
        if not 0 < self.max_flows <= 1 << 30:
            raise ValueError("max_flows must be in 1 .. 2^30")
        self.opts = encode_opts(key_flags(ports, proto, vlan, bidir), self.max_flows, hash_mask)
        lib = _lib.hip()
        out = dict(out or {})
        self.table = _buf(out, "table", (int(lib.zp_flow_table_bytes(self.max_flows)),), torch.uint8,
                          self.device)
        self.flows = _buf(out, "flows", (self.max_flows, STATE_DTYPE.itemsize), torch.uint8, self.device)
        self.init(stream)

    def init(self, stream=None):
        """Empties the table (F = 0, epoch = 0); `flows` is not touched. Enqueue-only."""
        rc = _lib.hip().zp_flow_table_init_device(self.table.data_ptr(), self.table.numel(),
                                                  self.opts.ctypes.data, _stream(stream, self.device))
        _lib.check(rc, "zp_flow_table_init_device")

    def update(self, arena, offs, lens, records, mask=None, want=("flow_of",), out=None, stream=None,
               check=True, opts=None):
        """One update by a parsed batch; returns TableUpdate(count, flow_of) of
        device tensors. count: int64 [8] = {F after the call, flows admitted,
        keyed frames, keyed bytes, refused flows, refused frames, the update's
        epoch, status}; status 1 means the table was not initialised with these
        options and nothing was done. flow_of: int32 [n], the table-wide flow
        number or -1 (None unless in `want`). mask, out ("count", "flow_of",
        "scratch") and check are as in aggregate(): check=False makes the call
        enqueue-only, so it captures into a graph. `opts` (an encode_opts
        array) replaces the table's own: tests pass a mismatch."""
        bad = set(want) - {"flow_of"}
        if bad:
            raise ValueError(f"unknown outputs {sorted(bad)}")
        for t in (arena, offs, lens, records, mask):
            if t is not None and not t.is_cuda:
                raise RuntimeError("flows.Table.update needs device tensors (no CPU fallback)")
        check_batch(arena, offs, lens, ((records, RECORD_BYTES),), bounds=check, stream=stream)
        dev = self.device
        if arena.device != dev:
            raise ValueError(f"the batch must be on {dev}")
        n = offs.numel()
        if n >= 1 << 31:
            raise ValueError("n must be below 2^31")
        if mask is not None and (mask.dtype != torch.int64 or mask.device != dev or
                                 not mask.is_contiguous() or mask.numel() < (n + 63) // 64):
            raise ValueError(f"mask must be a contiguous int64 tensor on {dev} with at least "
                             f"{(n + 63) // 64} words")
        out = dict(out or {})
        lib = _lib.hip()
        count = _buf(out, "count", (8,), torch.int64, dev)
        flow_of = _buf(out, "flow_of", (n,), torch.int32, dev) if "flow_of" in want else None
        scratch = _buf(out, "scratch", (int(lib.zp_flow_update_scratch_bytes(n)),), torch.uint8, dev)
        enc = self.opts if opts is None else opts
        rc = lib.zp_flow_update_device(
            arena.data_ptr(), offs.data_ptr(), lens.data_ptr(), records.data_ptr(), n, enc.ctypes.data,
            mask.data_ptr() if mask is not None else None, self.table.data_ptr(), self.table.numel(),
            self.flows.data_ptr(), flow_of.data_ptr() if flow_of is not None else None,
            count.data_ptr(), scratch.data_ptr(), scratch.numel(), _stream(stream, dev))
        _lib.check(rc, "zp_flow_update_device")
        if stream is not None:                # the allocator must not hand scratch on early
            scratch.record_stream(torch.cuda.ExternalStream(int(stream), device=dev))
        return TableUpdate(count, flow_of)

    def retire(self, max_idle=None, tcp_any=0, want=("retired", "remap"), out=None, stream=None,
               opts=None):
        """Retires the flows last seen max_idle or more updates before the
        latest one (None: never by age; 0: all) and those whose TCP flags meet
        tcp_any; returns TableRetire(count, retired, remap). count: int64 [2] =
        {F', flows retired} ({.., -1}: the table was not initialised with these
        options); retired: uint8 [max_flows, 64], the retired entries in
        ascending old number; remap: int32 [max_flows], old number -> new or
        -1, for the old F. Enqueue-only. out: "count", "retired", "remap",
        "scratch"."""
        bad = set(want) - {"retired", "remap"}
        if bad:
            raise ValueError(f"unknown outputs {sorted(bad)}")
        max_idle = IDLE_NEVER if max_idle is None else int(max_idle)
        if not 0 <= max_idle <= IDLE_NEVER or not 0 <= int(tcp_any) <= 0xFF:
            raise ValueError("max_idle must fit 32 bits and tcp_any 8 bits")
        dev, m = self.device, self.max_flows
        out = dict(out or {})
        lib = _lib.hip()
        count = _buf(out, "count", (2,), torch.int64, dev)
        retired = _buf(out, "retired", (m, STATE_DTYPE.itemsize), torch.uint8, dev) \
            if "retired" in want else None
        remap = _buf(out, "remap", (m,), torch.int32, dev) if "remap" in want else None
        scratch = _buf(out, "scratch", (int(lib.zp_flow_retire_scratch_bytes(m)),), torch.uint8, dev)
        enc = self.opts if opts is None else opts
        rc = lib.zp_flow_retire_device(
            enc.ctypes.data, self.table.data_ptr(), self.table.numel(), self.flows.data_ptr(),
            max_idle, int(tcp_any), retired.data_ptr() if retired is not None else None,
            remap.data_ptr() if remap is not None else None, count.data_ptr(), scratch.data_ptr(),
            scratch.numel(), _stream(stream, dev))
        _lib.check(rc, "zp_flow_retire_device")
        if stream is not None:
            scratch.record_stream(torch.cuda.ExternalStream(int(stream), device=dev))
        return TableRetire(count, retired, remap)

    def header(self):
        """(F, epoch) read back from the table's header: ONE SYNCHRONISATION."""
        h = self.table[:TABLE_HEADER_BYTES].cpu().numpy().view("<u8")
        return int(h[2]), int(h[3])

    def to_numpy(self):
        """The first F entries as a STATE_DTYPE array. Reads the header back:
        that is ONE SYNCHRONISATION with the device."""
        f, _ = self.header()
        f = min(f, self.max_flows)
        return self.flows.view(-1, STATE_DTYPE.itemsize)[:f].cpu().numpy().reshape(-1) \
            .view(STATE_DTYPE).copy()
