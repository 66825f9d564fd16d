"""The rule table of zp_classify_device restated with tests/select_ref.py (test
infrastructure): rule_of[i] is the first r for which select_ref.select_mask
holds with rules[r]; hits and the mask words follow from it with numpy.
Nothing about what a rule matches is new here.

Takes the encoded rules (an array of the zp_select layout, as
classify.encode_rules returns it), so what is checked is the ABI.
"""
import numpy as np

import select_ref as ref

RULE_NONE = 0xFFFFFFFF
HITS_DTYPE = np.dtype([("packets", "<u8"), ("bytes", "<u8")])


def rule_of(rules, cols, packed, lens):
    """uint32 [n]: the smallest matching rule index, RULE_NONE without one."""
    n = len(packed)
    out = np.full(n, RULE_NONE, np.uint32)
    for r in range(len(rules) - 1, -1, -1):
        out[ref.select_mask(rules[r:r + 1], cols, packed, lens)] = r
    return out


def hits(rule, lens, nrules):
    """HITS_DTYPE [nrules + 1]: packets and bytes per rule, unmatched frames last."""
    slot = np.where(rule == RULE_NONE, nrules, rule).astype(np.int64)
    h = np.zeros(nrules + 1, HITS_DTYPE)
    h["packets"] = np.bincount(slot, minlength=nrules + 1)
    ln = np.asarray(lens).astype(np.uint64)
    for k in np.unique(slot):
        h["bytes"][k] = ln[slot == k].sum(dtype=np.uint64)
    return h


def accepted(rule, nrules, accept=None):
    """bool [n]: frames whose rule is in `accept` (indices, RULE_NONE or
    nrules for "no rule"); None: matched any rule."""
    if accept is None:
        return rule != RULE_NONE
    acc = np.zeros(nrules + 1, bool)
    for r in accept:
        acc[nrules if r in (RULE_NONE, -1) else r] = True
    return acc[np.where(rule == RULE_NONE, nrules, rule).astype(np.int64)]


def mask_words(rule, nrules, accept=None):
    return ref.mask_words(accepted(rule, nrules, accept))
