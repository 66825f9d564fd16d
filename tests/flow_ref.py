"""The flow rule of zp_flow_aggregate_device restated in numpy and a dict (test
infrastructure): which frames are keyed, the 40-byte key built from the
oracle's columns (oracle.columns), the BIDIR swap, flows numbered by their
first frame, and the per-flow counters.

Takes the encoded zp_flow_opts (a one-element array of the struct's layout),
so what is checked is the ABI, not the facade. hash_mask is not looked at:
the results must not depend on it.
"""
import numpy as np

PORTS, PROTO, VLAN, BIDIR = 1, 2, 4, 8
NONE = 0xFFFFFFFF
F_IPV4, F_IPV6 = 1 << 2, 1 << 3

KEY_DTYPE = np.dtype([("src_addr", "u1", (16,)), ("dest_addr", "u1", (16,)), ("src_port", "<u2"),
                      ("dest_port", "<u2"), ("l4_proto", "u1"), ("ip_version", "u1"),
                      ("vlan", "<u2")])
FLOW_DTYPE = np.dtype([("key", KEY_DTYPE), ("first", "<u4"), ("last", "<u4"), ("packets", "<u4"),
                       ("tcp_flags", "u1"), ("pad", "u1", (3,)), ("bytes", "<u8")])


def keyed(packed, mask=None):
    """bool [n]: err == 0 and an outer IPv4 / IPv6 reader, and the mask's verdict."""
    w0 = np.asarray(packed["flags"], np.uint32)
    k = ((w0 >> 26) == 0) & ((w0 & (F_IPV4 | F_IPV6)) != 0)
    if mask is not None:
        k &= np.asarray(mask, bool)
    return k


def keys(cols, flags):
    """KEY_DTYPE [n]: every frame's key (meaningful for the keyed ones)."""
    n = len(cols["ip_version"])
    zero = np.zeros(n, np.uint16)
    sp = cols["src_port"] if flags & PORTS else zero
    dp = cols["dest_port"] if flags & PORTS else zero

    def endpoint(addr, port):                    # 18 bytes that compare as (address bytes, port)
        return np.concatenate([addr, (port >> 8).astype(np.uint8)[:, None],
                               (port & 0xFF).astype(np.uint8)[:, None]], axis=1)
    es, ed = endpoint(cols["src_addr"], sp), endpoint(cols["dest_addr"], dp)
    swap = np.zeros(n, bool)
    if flags & BIDIR and n:
        diff = es != ed
        at = diff.argmax(1)                      # the first byte that differs, if any does
        r = np.arange(n)
        swap = diff.any(1) & (es[r, at] > ed[r, at])
    k = np.zeros(n, KEY_DTYPE)
    k["src_addr"] = np.where(swap[:, None], cols["dest_addr"], cols["src_addr"])
    k["dest_addr"] = np.where(swap[:, None], cols["src_addr"], cols["dest_addr"])
    k["src_port"], k["dest_port"] = np.where(swap, dp, sp), np.where(swap, sp, dp)
    if flags & PROTO:
        k["l4_proto"] = cols["l4_proto"]
    k["ip_version"] = cols["ip_version"]
    if flags & VLAN:
        k["vlan"] = cols["vlan_tci"] & 0x0FFF
    return k


def aggregate(cols, packed, lens, opts, mask=None):
    """-> (flow_of uint32 [n], entries FLOW_DTYPE [F], count [F, keyed frames,
    keyed bytes, overflow]). cols: oracle.columns(...); packed: oracle.pack(...);
    opts: encoded zp_flow_opts; mask: bool [n] or None. With overflow the
    entries and flow_of returned are the whole, uncapped result."""
    o = opts[0]
    flags, max_flows = int(o["key_flags"]), int(o["max_flows"])
    n = len(packed)
    kd = keyed(packed, mask)
    idx = np.flatnonzero(kd)
    raw = keys(cols, flags).view(np.uint8).reshape(n, KEY_DTYPE.itemsize)
    flow_of = np.full(n, NONE, np.uint32)
    number, first = {}, []
    for i in idx:                                # ascending i: a flow's number is its order of discovery
        key = raw[i].tobytes()
        f = number.get(key)
        if f is None:
            f = number[key] = len(first)
            first.append(i)
        flow_of[i] = f
    ent = np.zeros(len(first), FLOW_DTYPE)
    ln = np.asarray(lens).astype(np.uint64)
    if len(first):
        f = flow_of[idx]
        ent["key"] = raw[first].reshape(-1).view(KEY_DTYPE)
        ent["first"] = first
        np.maximum.at(ent["last"], f, idx.astype(np.uint32))
        np.add.at(ent["packets"], f, 1)
        np.add.at(ent["bytes"], f, ln[idx])
        np.bitwise_or.at(ent["tcp_flags"], f, cols["tcp_flags"][idx])
    return flow_of, ent, [len(ent), len(idx), int(ln[idx].sum()), int(len(ent) > max_flows)]
