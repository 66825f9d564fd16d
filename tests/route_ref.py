"""The longest-prefix match of zp_route_device restated by brute force in
numpy (test infrastructure): the prefixes in ascending length, each assigned
to the routed frames of its version whose masked address equals it, so the
longest one is assigned last. No trie, nothing shared with the library.

Takes the encoded prefixes (an array of the zp_route_prefix layout, as
routes.encode_prefixes returns it) and oracle.columns output, so what is
checked is the ABI.
"""
import numpy as np

import select_ref as ref

NONE = 0xFFFFFFFF
F_IPV4, F_IPV6 = 1 << 2, 1 << 3


def routed(packed, only=None):
    """bool [n]: err == 0 and an outer IPv4 / IPv6 reader, and only's verdict."""
    w0 = np.asarray(packed["flags"], np.uint32)
    k = ((w0 >> 26) == 0) & ((w0 & (F_IPV4 | F_IPV6)) != 0)
    if only is not None:
        k &= np.asarray(only, bool)
    return k


def len_mask(length):
    """uint8 [16]: the first `length` bits set."""
    bits = np.zeros(128, np.uint8)
    bits[:length] = 1
    return np.packbits(bits)


def match_addrs(enc, addr, version, take=None):
    """(value uint32 [n], prefix int64 [n]) for addresses uint8 [n, 16] with
    their versions [n]: the value and the index in enc of the longest
    matching prefix (NONE / -1 without one). take: bool [n], who is looked up."""
    n = len(addr)
    value, prefix = np.full(n, NONE, np.uint32), np.full(n, -1, np.int64)
    addr = np.ascontiguousarray(np.asarray(addr, np.uint8).reshape(n, 16)).view("<u8")   # two words
    version = np.asarray(version)
    take = np.ones(n, bool) if take is None else np.asarray(take, bool)
    for k in np.argsort(enc["len"], kind="stable"):
        p = enc[k]
        m = len_mask(int(p["len"])).view("<u8")
        hit = take & (version == p["version"]) & ((addr & m) == p["addr"].view("<u8")).all(1)
        value[hit], prefix[hit] = p["value"], k
    return value, prefix


def match(enc, cols, packed, by="dest_addr", only=None):
    """match_addrs over a parsed batch: cols = oracle.columns(...), packed =
    oracle.pack(...); by: the address column; only: bool [n] or None."""
    return match_addrs(enc, cols[by], cols["ip_version"], routed(packed, only))


def value_of(enc, cols, packed, by="dest_addr", only=None):
    return match(enc, cols, packed, by, only)[0]


def mask_words(value):
    return ref.mask_words(value != NONE)


def depth(enc, prefix):
    """int [n]: the trie level the answering prefix lives at (1: a root entry,
    2: a /17../24, ...), 0 without an answer."""
    if len(enc) == 0:
        return np.zeros(len(prefix), np.int64)
    ln = enc["len"].astype(np.int64)[np.maximum(prefix, 0)]
    return np.where(prefix < 0, 0, 1 + np.maximum(0, (ln - 16 + 7) // 8))
