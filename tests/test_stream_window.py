"""The parse kernels' rolling stream window (zp_stream.h stream_window).

A tile's 16-B chunks are read as items of 64 chunks: a prologue of eight
loads, rounds of eight wait / consume / re-issue steps, and one of eight
straight-line epilogues for the items left; a tile of fewer than eight items
takes one right-sized group, a tile without chunks loads nothing, and the
frame-start masks are rebuilt every 64 items. The batches below put full
tiles at each of those item counts, for every alignment of the first frame,
and the same frames in other layouts; every case runs with record codes off
(zp_parse_kernel), with record codes on (zp_parse_slots_kernel +
zp_rec_expand_kernel) and through zp_parse_batch_columns_device
(zp_parse_columns_kernel), against the CPU oracle byte for byte.

The item count of a tile is computed here from the descriptors,
sum((len + (offs & 15) + 15) >> 4 for len >= 64) chunks in items of 64, and
asserted when a batch is built (the CPU test builds every batch).
"""
import functools

import numpy as np
import pytest

import oracle as orc
from test_gpu_parity import _udp4
from test_gpu_paths import run_path, slots  # noqa: F401  (slots: a fixture)

ITEM_COUNTS = [0, 1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 129]
MIXED = ["ragged", "short_and_long", "one_jumbo"]
LAYOUTS = ["gapped", "reversed", "shuffled"]
PATHS = ["plain", "codes", "fused"]     # zp_set_record_slots 2, 1; the fused column kernel
SHORT = 60          # a frame below 64 B owns no chunks
JUMBO = 9000
TILES = 2           # full tiles per item-count batch


@functools.lru_cache(maxsize=None)
def frame(length, k):
    """A UDP/IPv4 frame of `length` bytes; every 7th variant fails its checksum."""
    return _udp4(length, 1000 * k + length, valid=k % 7 != 3)


def chunks(length, off):
    return (length + (off & 15) + 15) >> 4 if length >= 64 else 0


def tile_lengths(items, off):
    """64 frame lengths, back to back from offset `off`, whose chunks make
    exactly `items` stream items: the largest of 1,500 / 576 / 64 B that
    still fits, one after another (tiles of more than 90 items start from
    9,000-B frames), and 60-B filler frames, which own no chunks, for the
    rest."""
    sizes = ([JUMBO] if items > 90 else []) + [1500, 576, 64]
    room = 64 * items
    out = []
    while len(out) < 64:
        fit = [s for s in sizes if chunks(s, off) <= room]
        s = fit[0] if fit else SHORT
        room -= chunks(s, off)
        off += s
        out.append(s)
    return out


def tile_items(offs, lens):
    """Stream items of each full or ragged tile of 64 descriptors."""
    c = [chunks(int(l), int(o)) for o, l in zip(offs, lens)]
    return [(sum(c[t:t + 64]) + 63) >> 6 for t in range(0, len(c), 64)]


class Case:
    def __init__(self, lens, align=0, pick=None):
        frames = [frame(l, i % 11) for i, l in enumerate(lens)]
        self.lens = np.array([len(f) for f in frames], np.uint32)
        self.offs = (align + np.concatenate([[0], np.cumsum(self.lens[:-1], dtype=np.int64)])
                     ).astype(np.uint64)
        self.arena = np.zeros(int(self.offs[-1] + self.lens[-1]), np.uint8)   # tight end
        for o, f in zip(self.offs, frames):
            self.arena[int(o):int(o) + len(f)] = np.frombuffer(f, np.uint8)
        if pick is not None:
            self.offs, self.lens = self.offs[pick], self.lens[pick]
        self.want, self.wext = orc.parse_batch(self.arena, self.offs, self.lens)
        self.packed = orc.pack(self.want, self.wext).view(np.uint8).reshape(-1, 8)
        self.cols = orc.columns(self.arena, self.offs, self.lens, self.want)


@functools.lru_cache(maxsize=None)
def count_case(items, align):
    """TILES full tiles of exactly `items` items each, the first frame at
    arena offset `align` (0-15)."""
    lens, off = [], align
    for _ in range(TILES):
        t = tile_lengths(items, off)
        lens += t
        off += sum(t)
    c = Case(tuple(lens), align)
    assert tile_items(c.offs, c.lens) == [items] * TILES, (items, align)
    if items:
        assert {64, 576, 1500} & set(lens)
    # good and failing checksums both occur among the frames that own chunks
    errs = c.want["err"][c.lens >= 64]
    assert items == 0 or ((errs == 0).any() and (errs != 0).any())
    return c


def mixed_lengths(kind):
    if kind == "ragged":               # two full tiles and 37 frames
        return [1500, 64, 576, 333, 64] * 33
    if kind == "short_and_long":       # frames without chunks between long ones
        return [SHORT, 1500, SHORT, SHORT, 576, 64, 48, 1500] * 16 + [SHORT] * 64 + [576, SHORT] * 8
    if kind == "one_jumbo":            # one 9,000-B frame among 64-B frames, per tile
        return ([64] * 20 + [JUMBO] + [64] * 43) + ([JUMBO] + [64] * 63) + ([64] * 63 + [JUMBO])
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def mixed_case(kind):
    c = Case(tuple(mixed_lengths(kind)))
    it = tile_items(c.offs, c.lens)
    if kind == "ragged":
        assert len(c.lens) % 64 == 37 and it[-1] > 8
    elif kind == "short_and_long":
        assert it[2] == 0 and (c.lens[:64] < 64).sum() == 32 and it[0] > 8 and 0 < it[3] < 8
    else:
        assert min(it) > 8 and (c.lens == JUMBO).sum() == 3
    return c


def base_lengths(name):
    """The frame lengths of a named batch: "n<items>" or a mixed one."""
    if name.startswith("n"):
        lens, off = [], 0
        for _ in range(TILES):
            t = tile_lengths(int(name[1:]), off)
            lens += t
            off += sum(t)
        return lens
    return mixed_lengths(name)


BATCHES = [f"n{k}" for k in ITEM_COUNTS] + MIXED


@functools.lru_cache(maxsize=None)
def layout_case(name, layout):
    """The frames of a batch in another order: every second frame (the
    others are gaps in the arena), the descriptors reversed, or shuffled."""
    lens = base_lengths(name)
    n = len(lens)
    if layout == "gapped":
        lens = [l for l in lens for _ in (0, 1)]          # each frame twice, the copy skipped
        pick = np.arange(0, 2 * n, 2)
    elif layout == "reversed":
        pick = np.arange(n)[::-1].copy()
    elif layout == "shuffled":
        pick = np.random.default_rng(n).permutation(n)
    else:
        raise ValueError(layout)
    c = Case(tuple(lens), 0, pick)
    assert len(c.lens) == n <= 8192
    if layout == "gapped":
        assert (np.diff(c.offs.astype(np.int64)) > c.lens[:-1]).all()
    return c


def run_and_check(zp, slots, c, shift, paths=PATHS):
    for path in paths:
        rec, ext, cols = run_path(zp, slots, path, c.arena, c.offs, c.lens, base_shift=shift)
        g = rec.view(np.uint8).reshape(-1, 8)
        diff = np.nonzero((g != c.packed).any(1))[0]
        assert len(diff) == 0, (path, shift, len(diff), diff[:5])
        assert zp.records.ext_match(ext, c.wext, c.want), (path, shift)
        if cols is not None:
            for name, wantcol in c.cols.items():
                assert np.array_equal(cols[name], wantcol), (path, shift, name)


# ---- CPU: the batches are what they claim -----------------------------------

@pytest.mark.parametrize("items", ITEM_COUNTS)
def test_item_count_batches_cpu(items):
    for align in range(16):
        c = count_case(items, align)
        assert len(c.lens) == 64 * TILES and int(c.offs[0]) == align


def test_other_batches_cpu():
    for kind in MIXED:
        mixed_case(kind)
    for name in BATCHES:
        for layout in LAYOUTS:
            layout_case(name, layout)


# ---- GPU ----------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("items", ITEM_COUNTS)
def test_item_counts(zp, slots, items):
    """Full tiles of exactly `items` stream items, the first frame at each
    alignment 0-15 (the frames are chosen per alignment, so the count holds
    at each)."""
    for align in range(16):
        c = count_case(items, align)
        # the arena already starts `align` bytes in: the device copy is 16-B aligned
        run_and_check(zp, slots, c, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", MIXED)
def test_mixed_tiles(zp, slots, kind):
    c = mixed_case(kind)
    for shift in range(16):
        run_and_check(zp, slots, c, shift)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", BATCHES)
def test_layouts(zp, slots, name, layout):
    c = layout_case(name, layout)
    for shift in range(16):
        run_and_check(zp, slots, c, shift)
