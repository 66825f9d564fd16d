"""Classify: a first-match rule table over parsed frames on the device
(zp_classify_compile, zp_classify_device; semantics in include/zero_packet.h).

    S = select.Select
    table = classify.RuleTable([S(ok=True).where("l4_proto", eq=6).where("dest_port", eq=443),
                                S(ok=True).where("src_addr", prefix="10.0.0.0/8")
                                .where("ip_version", eq=4),
                                S(ok=False)], device="cuda:0")
    c = table.run(arena, offs, lens, records)
    c.rule_of      # int32 [n]: the first rule that matches frame i, RULE_NONE (-1 as int32) if none
    table.hits     # int64 [nrules + 1, 2]: {packets, bytes} per rule, unmatched frames last;
                   # every run adds to it (table.reset_hits() zeroes it)
    c.mask         # the words select.run writes: frames whose rule is in accept= (default: any rule)

A rule is a select.Select and matches exactly the frames select.run would
select with it; the rules are tried in order and the first match wins.
"""
import collections

import numpy as np
import torch

from . import _lib
from .batch import check_batch
from .records import RECORD_BYTES
from .select import SELECT_DTYPE, Select, _ptr, _stream

MAX_RULES = 256                    # ZP_CLASSIFY_MAX_RULES
RULE_NONE = 0xFFFFFFFF             # ZP_RULE_NONE
HITS_DTYPE = np.dtype([("packets", "<u8"), ("bytes", "<u8")])      # zp_rule_hits

Classified = collections.namedtuple("Classified", "rule_of hits mask status")


def encode_rules(rules):
    """The zp_select array zp_classify_compile takes (SELECT_DTYPE [len(rules)])."""
    rules = list(rules)
    for r in rules:
        if not isinstance(r, Select):
            raise TypeError("rules must be select.Select objects")
    enc = np.zeros(len(rules), SELECT_DTYPE)
    for k, r in enumerate(rules):
        enc[k] = r.encode()[0]
    return enc


def compile_rules(enc):
    """zp_classify_compile on an encoded rule array -> (table bytes as a
    uint8 array, needs_frames). Host only; raises on a refusal."""
    lib = _lib.hip()
    enc = np.ascontiguousarray(enc, SELECT_DTYPE)
    nbytes = int(lib.zp_classify_table_bytes(len(enc)))
    if nbytes == 0:
        raise ValueError(f"a rule table holds 1..{MAX_RULES} rules, not {len(enc)}")
    table = np.zeros(nbytes // 8, np.uint64)          # 8-byte aligned
    rc = lib.zp_classify_compile(enc.ctypes.data, len(enc), table.ctypes.data, nbytes)
    _lib.check(rc, "zp_classify_compile")
    return table.view(np.uint8), bool(rc)


def accept_words(accept, nrules):
    """The `accept` bitmap of zp_classify_device from an iterable of rule
    indices (RULE_NONE or nrules: the frames no rule matches)."""
    words = np.zeros((nrules + 64) // 64, np.uint64)
    for r in accept:
        r = nrules if int(r) in (RULE_NONE, -1) else int(r)
        if not 0 <= r <= nrules:
            raise ValueError(f"accept: rule index {r} out of range")
        words[r >> 6] |= np.uint64(1 << (r & 63))
    return words


class RuleTable:
    """`rules` (select.Select objects, in priority order) compiled and copied
    to `device`, with a persistent hits tensor (int64 [nrules + 1, 2])."""

    def __init__(self, rules, device):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("classify.RuleTable needs a GPU device (no CPU fallback)")
        self.rules = encode_rules(rules)
        self.nrules = len(self.rules)
        host, self.needs_frames = compile_rules(self.rules)
        self.table_host = host
        self.table = torch.from_numpy(host.copy()).to(self.device)
        self.hits = torch.zeros((self.nrules + 1, 2), dtype=torch.int64, device=self.device)

    def reset_hits(self):
        self.hits.zero_()

    def hits_numpy(self):
        """The counters as a structured array (HITS_DTYPE [nrules + 1]); entry
        nrules counts the frames no rule matched. Synchronises."""
        return self.hits.cpu().numpy().view(np.uint64).reshape(-1).view(HITS_DTYPE).copy()

    def run(self, arena, offs, lens, records, want=("rule_of", "hits", "mask"), accept=None,
            out=None, stream=None, check=True):
        """Classifies a parsed batch; returns Classified(rule_of, hits, mask,
        status) of device tensors (those not in `want` are None). rule_of:
        int32 [n] (RULE_NONE reads as -1); hits: self.hits, added to; mask:
        int64 [ceil(n / 64)], frames whose rule is in `accept` (an iterable of
        rule indices, RULE_NONE for "no rule"; default: any rule); status:
        int64 [1], 0, or 1 when the kernel refused the table. `out` may hold
        preallocated tensors under the same names. A record-only table takes
        arena=None, offs=None. check=True reads status back (one
        synchronisation) and raises on 1, and runs the descriptor bounds
        reduction of batch.parse_batch; check=False is enqueue-only."""
        bad = set(want) - {"rule_of", "hits", "mask"}
        if bad:
            raise ValueError(f"unknown outputs {sorted(bad)}")
        for t in (arena, offs, lens, records):
            if t is not None and not t.is_cuda:
                raise RuntimeError("classify needs device tensors (no CPU fallback)")
        if self.needs_frames and (arena is None or offs is None or lens is None):
            raise ValueError("a table whose rules have terms needs arena, offs and lens")
        if "hits" in want and lens is None:
            raise ValueError("hits need lens")
        dev = records.device
        n = records.numel() * records.element_size() // RECORD_BYTES
        if arena is not None and offs is not None and lens is not None:
            check_batch(arena, offs, lens, ((records, RECORD_BYTES),),
                        bounds=check and self.needs_frames, stream=stream)
        elif not records.is_contiguous():
            raise ValueError("records must be contiguous")
        if lens is not None and (lens.dtype != torch.int32 or lens.numel() != n or
                                 not lens.is_contiguous()):
            raise ValueError(f"lens must be contiguous int32 with {n} entries")
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
        rule_of = buf("rule_of", (n,), torch.int32) if "rule_of" in want else None
        mask = buf("mask", ((n + 63) // 64,), torch.int64) if "mask" in want else None
        hits = None
        if "hits" in want:
            hits = out.get("hits", self.hits)
            if hits.dtype != torch.int64 or hits.device != dev or not hits.is_contiguous() or \
                    hits.numel() < 2 * (self.nrules + 1):
                raise ValueError("hits must be a contiguous int64 tensor of nrules + 1 pairs")
        status = buf("status", (1,), torch.int64)
        acc = accept_words(accept, self.nrules) if accept is not None else None
        frames = self.needs_frames
        rc = _lib.hip().zp_classify_device(
            _ptr(arena) if frames else None, _ptr(offs) if frames else None, _ptr(lens),
            records.data_ptr(), n, self.table.data_ptr(), self.table.numel(), self.nrules,
            acc.ctypes.data if acc is not None else None, _ptr(rule_of), _ptr(hits), _ptr(mask),
            status.data_ptr(), _stream(stream, dev))
        _lib.check(rc, "zp_classify_device")
        if check and int(status[0]) != 0:
            raise RuntimeError("zp_classify_device: the kernel refused the table (status 1): it "
                               "is not the compiled form of this rule count")
        return Classified(rule_of, hits, mask, status)


def run(table, arena, offs, lens, records, **kw):
    """table.run(arena, offs, lens, records, **kw)."""
    return table.run(arena, offs, lens, records, **kw)

