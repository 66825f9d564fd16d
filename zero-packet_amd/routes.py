"""Route: longest-prefix match of a frame's outer address on the device
(zp_route_compile, zp_route_device; semantics in include/zero_packet.h).

    table = routes.RouteTable([("10.0.0.0/8", 1), ("10.1.0.0/16", 2), ("2001:db8::/32", 3),
                               ("0.0.0.0/0", 0)], device="cuda:0")
    r = table.run(arena, offs, lens, records)            # by="dest_addr"
    r.value_of     # int32 [n]: the value of the longest matching prefix of the frame's IP
                   # version, ROUTE_NONE (-1 as int32) if none or the frame is not routed
    r.mask         # the words select.run writes: frames with a match
    table.lookup("10.1.2.3")                             # the same walk on the host: 2

The version is part of the match: an IPv4 prefix never matches an IPv6 frame.
"""
import collections
import ipaddress

import numpy as np
import torch

from . import _lib
from .batch import check_batch
from .columns import INDEX
from .records import RECORD_BYTES
from .select import _ptr, _stream

ROUTE_NONE = 0xFFFFFFFF            # ZP_ROUTE_NONE
VALUE_MAX = 0x7FFFFFFE             # ZP_ROUTE_VALUE_MAX
MAX_PREFIXES = 1 << 20             # ZP_ROUTE_MAX_PREFIXES
PREFIX_DTYPE = np.dtype([("addr", "u1", (16,)), ("len", "u1"), ("version", "u1"),
                         ("pad", "u1", (2,)), ("value", "<u4")])      # zp_route_prefix

Routed = collections.namedtuple("Routed", "value_of mask status")


def encode_prefixes(prefixes, strict=True):
    """The zp_route_prefix array zp_route_compile takes (PREFIX_DTYPE) from
    (network, value) pairs or a {network: value} mapping; a network is a CIDR
    string or an ipaddress network. strict=False masks host bits
    ("10.1.2.3/8" is 10.0.0.0/8) where strict=True raises ValueError."""
    if isinstance(prefixes, np.ndarray) and prefixes.dtype == PREFIX_DTYPE:
        return np.ascontiguousarray(prefixes)
    pairs = list(prefixes.items()) if hasattr(prefixes, "items") else list(prefixes)
    enc = np.zeros(len(pairs), PREFIX_DTYPE)
    for k, (net, value) in enumerate(pairs):
        if not isinstance(net, (ipaddress.IPv4Network, ipaddress.IPv6Network)):
            net = ipaddress.ip_network(net, strict=strict)
        if not 0 <= int(value) <= VALUE_MAX:
            raise ValueError(f"prefix {k}: value {value} not in 0..VALUE_MAX")
        packed = net.network_address.packed
        enc[k]["addr"][:len(packed)] = np.frombuffer(packed, np.uint8)
        enc[k]["len"], enc[k]["version"], enc[k]["value"] = net.prefixlen, net.version, int(value)
    return enc


def compile_prefixes(enc):
    """zp_route_compile on an encoded prefix array -> the table's bytes as a
    uint8 array. Host only; raises on a refusal."""
    lib = _lib.hip()
    enc = np.ascontiguousarray(enc, PREFIX_DTYPE)
    nbytes = int(lib.zp_route_table_bytes(enc.ctypes.data, len(enc)))
    if nbytes == 0:
        raise ValueError("zp_route_table_bytes: " + lib.zp_last_error().decode(errors="replace"))
    table = np.zeros(nbytes // 8, np.uint64)          # 8-byte aligned
    _lib.check(lib.zp_route_compile(enc.ctypes.data, len(enc), table.ctypes.data, nbytes),
               "zp_route_compile")
    return table.view(np.uint8)


def lookup_host(table, addr):
    """zp_route_lookup_host: one address (a string, an ipaddress address, or
    (16 bytes, version)) through a compiled table held in host memory."""
    if isinstance(addr, tuple):
        raw, version = bytes(addr[0]), int(addr[1])
    else:
        a = ipaddress.ip_address(addr)
        raw, version = a.packed, a.version
    buf = np.zeros(16, np.uint8)
    buf[:len(raw)] = np.frombuffer(raw, np.uint8)
    table = np.ascontiguousarray(table, np.uint8)
    return int(_lib.hip().zp_route_lookup_host(table.ctypes.data, table.size, buf.ctypes.data,
                                               version))


class RouteTable:
    """`prefixes` (see encode_prefixes) compiled and copied to `device`."""

    def __init__(self, prefixes, device, strict=True):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("routes.RouteTable needs a GPU device (no CPU fallback)")
        self.prefixes = encode_prefixes(prefixes, strict=strict)
        self.table_host = compile_prefixes(self.prefixes)
        self.table = torch.from_numpy(self.table_host.copy()).to(self.device)

    def lookup(self, addr):
        """The value of the longest prefix that matches `addr`, ROUTE_NONE if
        none: the kernel's walk over the host copy."""
        return lookup_host(self.table_host, addr)

    def run(self, arena, offs, lens, records, by="dest_addr", only=None, want=("value_of", "mask"),
            out=None, stream=None, check=True):
        """Routes a parsed batch by its outer `by` address ("dest_addr" or
        "src_addr"); returns Routed(value_of, mask, status) of device tensors
        (those not in `want` are None). value_of: int32 [n] (ROUTE_NONE reads
        as -1); mask: int64 [ceil(n / 64)], the frames with a match; status:
        int64 [1], 0, or 1 when the kernel refused the table. only: the mask
        words of select.run / classify (int64 [ceil(n / 64)]): frames whose
        bit is clear are not routed. `out` may hold preallocated tensors under
        the same names. check=True reads status back (one synchronisation) and
        raises on 1, and runs the descriptor bounds reduction of
        batch.parse_batch; check=False is enqueue-only."""
        bad = set(want) - {"value_of", "mask"}
        if bad:
            raise ValueError(f"unknown outputs {sorted(bad)}")
        if by not in ("dest_addr", "src_addr"):
            raise ValueError("by must be 'dest_addr' or 'src_addr'")
        for t in (arena, offs, lens, records, only):
            if t is not None and not t.is_cuda:
                raise RuntimeError("routes needs device tensors (no CPU fallback)")
        if arena is None or offs is None or lens is None:
            raise ValueError("route reads frames: it needs arena, offs and lens")
        dev = records.device
        n = records.numel() * records.element_size() // RECORD_BYTES
        check_batch(arena, offs, lens, ((records, RECORD_BYTES),), bounds=check, stream=stream)
        words = (n + 63) // 64
        if only is not None and (only.dtype != torch.int64 or only.device != dev or
                                 not only.is_contiguous() or only.numel() < words):
            raise ValueError(f"only must be a contiguous int64 tensor on {dev} with at least "
                             f"{words} words")
        out = dict(out or {})

        def buf(name, shape, dtype):
            t = out.get(name)
            if t is None:
                return torch.empty(shape, dtype=dtype, device=dev)
            if t.dtype != dtype or t.device != dev or not t.is_contiguous() or \
                    t.numel() < int(np.prod(shape)):
                raise ValueError(f"out[{name!r}] must be a contiguous {dtype} tensor on {dev} "
                                 f"with at least {int(np.prod(shape))} elements")
            return t
        value_of = buf("value_of", (n,), torch.int32) if "value_of" in want else None
        mask = buf("mask", (words,), torch.int64) if "mask" in want else None
        status = buf("status", (1,), torch.int64)
        rc = _lib.hip().zp_route_device(
            arena.data_ptr(), offs.data_ptr(), lens.data_ptr(), records.data_ptr(), n,
            self.table.data_ptr(), self.table.numel(), INDEX[by], _ptr(only), _ptr(value_of),
            _ptr(mask), status.data_ptr(), _stream(stream, dev))
        _lib.check(rc, "zp_route_device")
        if check and int(status[0]) != 0:
            raise RuntimeError("zp_route_device: the kernel refused the table (status 1): it is "
                               "not a compiled route table of this size")
        return Routed(value_of, mask, status)


def run(table, arena, offs, lens, records, **kw):
    """table.run(arena, offs, lens, records, **kw)."""
    return table.run(arena, offs, lens, records, **kw)
