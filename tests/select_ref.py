"""The selection rule of zp_select_device restated in numpy (test
infrastructure): a frame is selected when the record predicate, the length
bounds and every term hold, a term's value being the entry the oracle's
columns (oracle.columns) hold for that column.

Takes the encoded zp_select (a one-element array of the struct's layout, as
Select.encode() returns it), so what is checked is the ABI, not the facade.
"""
import numpy as np

import oracle as orc

MASK_EQ, MASK_NE, RANGE, NOT_RANGE = 0, 1, 2, 3
ERR_ANY, ERR_NONZERO = -1, -2
F_MASK = 0x00FFFFFF


def select_mask(sel, cols, packed, lens):
    """bool [n]. sel: encoded zp_select; cols: oracle.columns(...) (only the
    terms' columns are read; may be None without terms); packed: the ABI's
    8-B records (oracle.pack); lens: uint32 [n] or None."""
    s = sel[0]
    w0 = np.asarray(packed["flags"], np.uint32)
    f, e = w0 & F_MASK, (w0 >> 26).astype(np.int64)
    m = ((f & s["flags_all"]) == s["flags_all"]) & ((f & s["flags_none"]) == 0)
    if s["flags_any"]:
        m &= (f & s["flags_any"]) != 0
    err = int(s["err"])
    if err == ERR_NONZERO:
        m &= e != 0
    elif err != ERR_ANY:
        m &= e == err
    if lens is not None:
        ln = np.asarray(lens).astype(np.uint64)
        m &= (ln >= int(s["min_len"])) & (ln <= int(s["max_len"]))
    for k in range(int(s["nterms"])):
        t = s["terms"][k]
        name, dt, w = orc.COLUMN_SPEC[int(t["col"])]
        width = w * np.dtype(dt).itemsize
        col = np.ascontiguousarray(cols[name])
        a, b = bytes(t["a"][:width]), bytes(t["b"][:width])
        op = int(t["op"])
        if op in (MASK_EQ, MASK_NE):
            v = col.view(np.uint8).reshape(len(col), width)        # little-endian host
            hit = ((v & np.frombuffer(b, np.uint8)) == np.frombuffer(a, np.uint8)).all(1)
        else:
            assert w == 1, "range terms are for scalar columns"
            v = col.astype(np.uint64)
            hit = (v >= int.from_bytes(a, "little")) & (v <= int.from_bytes(b, "little"))
        m &= hit if op in (MASK_EQ, RANGE) else ~hit
    return m


def compact(mask, lens):
    """-> (idx uint32 [c], packed_offs uint64 [c], count, total bytes)."""
    idx = np.flatnonzero(mask).astype(np.uint32)
    if lens is None:
        return idx, np.zeros(len(idx), np.uint64), len(idx), 0
    sl = np.asarray(lens).astype(np.uint64)[idx]
    packed = np.concatenate([[0], np.cumsum(sl)[:-1]]).astype(np.uint64) if len(idx) else \
        np.zeros(0, np.uint64)
    return idx, packed, len(idx), int(sl.sum())


def mask_words(mask):
    """The verdicts as the kernel's words: bit i % 64 of word i / 64."""
    n = len(mask)
    bits = np.zeros((n + 63) // 64 * 64, np.uint8)
    bits[:n] = mask
    return np.packbits(bits.reshape(-1, 8), axis=1, bitorder="little").reshape(-1).view("<u8")


def packed_bytes(arena, offs, lens, idx):
    """The selected frames back to back."""
    arena = np.asarray(arena, np.uint8)
    parts = [arena[int(offs[i]):int(offs[i]) + int(lens[i])] for i in idx]
    return np.concatenate(parts) if parts else np.zeros(0, np.uint8)
