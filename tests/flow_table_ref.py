"""The rule of zp_flow_update_device / zp_flow_retire_device restated in Python
with a dict and a list (test infrastructure), on flow_ref.keyed / flow_ref.keys.

Takes the encoded zp_flow_opts, like flow_ref. hash_mask is not looked at: the
results must not depend on it.
"""
import numpy as np

import flow_ref as ref

NONE = ref.NONE
IDLE_NEVER = 0xFFFFFFFF
STATE_DTYPE = np.dtype([("key", ref.KEY_DTYPE), ("first_epoch", "<u4"), ("last_epoch", "<u4"),
                        ("packets_flags", "<u8"), ("bytes", "<u8")])
PACKETS_MASK = (1 << 56) - 1


class Table:
    """number: key bytes -> flow number; entries: one dict per flow, in order."""

    def __init__(self, opts):
        o = opts[0]
        self.flags, self.max_flows = int(o["key_flags"]), int(o["max_flows"])
        self.number, self.entries, self.epoch = {}, [], 0

    def update(self, cols, packed, lens, mask=None):
        """-> (flow_of uint32 [n], count: the 8 words). Frames are walked in
        ascending order: a new key's rank is its order of discovery, which is
        the order of its first frame."""
        n = len(packed)
        kd = ref.keyed(packed, mask)
        raw = ref.keys(cols, self.flags).view(np.uint8).reshape(n, ref.KEY_DTYPE.itemsize)
        flow_of = np.full(n, NONE, np.uint32)
        f0, e = len(self.entries), self.epoch
        new, refused = {}, set()                     # this batch's new keys -> rank
        keyed_frames = keyed_bytes = refused_frames = 0
        for i in np.flatnonzero(kd):
            key = raw[i].tobytes()
            keyed_frames += 1
            keyed_bytes += int(lens[i])
            f = self.number.get(key)
            if f is None:
                r = new.setdefault(key, len(new))
                if f0 + r < self.max_flows:          # admitted as F0 + r
                    f = self.number[key] = f0 + r
                    self.entries.append(dict(key=key, first_epoch=e, last_epoch=e, packets=0, flags=0,
                                             bytes=0))
                    assert len(self.entries) == f + 1
                else:
                    refused.add(key)
                    refused_frames += 1
                    continue
            ent = self.entries[f]
            ent["packets"] += 1
            ent["bytes"] += int(lens[i])
            ent["flags"] |= int(cols["tcp_flags"][i])
            ent["last_epoch"] = e
            flow_of[i] = f
        self.epoch += 1
        f1 = len(self.entries)
        return flow_of, [f1, f1 - f0, keyed_frames, keyed_bytes, len(refused), refused_frames, e, 0]

    def retire(self, max_idle=IDLE_NEVER, tcp_any=0):
        """-> (retired STATE_DTYPE array, remap uint32 [old F], count [F', retired])."""
        keep, gone = [], []
        remap = np.full(len(self.entries), NONE, np.uint32)
        for f, ent in enumerate(self.entries):
            idle = max_idle != IDLE_NEVER and self.epoch - 1 - ent["last_epoch"] >= max_idle
            if idle or ent["flags"] & tcp_any:
                gone.append(ent)
            else:
                remap[f] = len(keep)
                keep.append(ent)
        self.entries = keep
        self.number = {ent["key"]: f for f, ent in enumerate(keep)}
        return states(gone), remap, [len(keep), len(gone)]

    def states(self):
        return states(self.entries)


def states(entries):
    """The entries as the device holds them (STATE_DTYPE)."""
    m = len(entries)
    out = np.zeros(m, STATE_DTYPE)
    out["key"] = np.frombuffer(b"".join(e["key"] for e in entries), ref.KEY_DTYPE)
    out["first_epoch"] = np.fromiter((e["first_epoch"] for e in entries), np.uint32, m)
    out["last_epoch"] = np.fromiter((e["last_epoch"] for e in entries), np.uint32, m)
    out["packets_flags"] = np.fromiter((e["packets"] | e["flags"] << 56 for e in entries), np.uint64, m)
    out["bytes"] = np.fromiter((e["bytes"] for e in entries), np.uint64, m)
    return out


def piece(b, lo, hi):
    """(cols, packed, lens) of frames [lo, hi) of a test_select.Batch."""
    return {k: v[lo:hi] for k, v in b.cols.items()}, b.packed[lo:hi], b.lens[lo:hi]
