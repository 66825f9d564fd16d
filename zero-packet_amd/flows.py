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
