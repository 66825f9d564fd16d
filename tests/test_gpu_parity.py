"""GPU parity: the HIP path (through the C ABI) against the oracle.

Bit-exact on every record byte (integer/byte work). Covers the reference's
golden packets, all five synthetic configs, mutation fuzz, odd layouts
(gaps, overlap, reverse order, odd base address), edge lengths, jumbo IPv6
frames (exact u32-wrap checksum path), the host-buffer path, and full-size
C3 properties.
"""
import ctypes
import random

import numpy as np
import pytest

import oracle as orc
from test_oracle_fuzz import mutate
from test_oracle_golden import ERR, check_expect

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def pack(frames, base_pad=0, gap=0):
    """frames -> host (arena, offs, lens), frames back to back (plus gap)."""
    offs, pos = [], base_pad
    for f in frames:
        offs.append(pos)
        pos += len(f) + gap
    arena = np.zeros(pos + 64, np.uint8)
    for o, f in zip(offs, frames):
        arena[o:o + len(f)] = np.frombuffer(bytes(f), np.uint8)
    return arena, np.array(offs, np.uint64), np.array([len(f) for f in frames], np.uint32)


def gpu_parse(zp, arena, offs, lens, base_shift=0):
    d = dev()
    a = torch.zeros(len(arena) + base_shift + 16, dtype=torch.uint8, device=d)
    a[base_shift:base_shift + len(arena)] = torch.from_numpy(np.asarray(arena, np.uint8)).to(d)
    o = torch.from_numpy(np.asarray(offs, np.int64) + base_shift).to(d)
    l_ = torch.from_numpy(np.asarray(lens, np.uint32).astype(np.int32)).to(d)
    r, e = zp.batch.parse_batch(a, o, l_)
    torch.cuda.synchronize()
    return zp.batch.records_to_numpy(r, e)


def assert_same(got, got_ext, want, want_ext):
    """Records byte-identical; the extension chains the records flag
    identical (records.ext_match; other ext entries are unspecified)."""
    g = got.view(np.uint8).reshape(-1, 8)
    w = orc.pack(want, want_ext).view(np.uint8).reshape(-1, 8)   # the oracle's records, packed
    diff = np.nonzero((g != w).any(1))[0]
    assert len(diff) == 0, (f"{len(diff)} records differ; first {diff[:5]}",
                            got[diff[:3]], want[diff[:3]])
    from importlib import import_module
    assert import_module("zero-packet_amd").records.ext_match(got_ext, want_ext, want)


# ---- golden packets ------------------------------------------------------

def test_golden_batch(zp, golden):
    frames = [bytes.fromhex(fx["bytes"]) for fx in golden["fixtures"]]
    for shift in (0, 1, 3, 7):
        arena, offs, lens = pack(frames)
        got, gext = gpu_parse(zp, arena, offs, lens, base_shift=shift)
        want, wext = orc.parse_batch(arena, offs, lens)
        assert_same(got, gext, want, wext)
        for fx, f, r, e in zip(golden["fixtures"], frames, got, gext.T):
            check_expect(zp, f, r, e, fx["expect"])


def test_golden_parse_one(zp, golden):
    """PacketParser.parse (zp_parse_one: host frame -> GPU -> record)."""
    for fx in golden["fixtures"]:
        f = bytes.fromhex(fx["bytes"])
        if fx["expect"]["ok"]:
            p = zp.PacketParser.parse(f)
            assert p.ethernet is not None
        else:
            with pytest.raises(zp.ZeroPacketError) as ei:
                zp.PacketParser.parse(f)
            if "err" in fx["expect"]:
                assert ei.value.code == ERR[fx["expect"]["err"]]


# ---- synthetic configs ---------------------------------------------------

@pytest.mark.parametrize("cfg,n", [("c1", 50000), ("c3", 40000), ("c4", 40000),
                                   ("c5", 60000), ("c6", 60000)])
def test_synthetic_configs_exact(zp, cfg, n):
    arena, offs, lens = zp.batch.generate(cfg, n, first=99991, device=dev())
    r, e = zp.batch.parse_batch(arena, offs, lens)
    torch.cuda.synchronize()
    got, gext = zp.batch.records_to_numpy(r, e)
    want, wext = orc.parse_batch(arena.cpu().numpy(), offs.cpu().numpy(), lens.cpu().numpy())
    assert (want["err"] == 0).all()
    assert_same(got, gext, want, wext)


@pytest.mark.parametrize("cfg", ["c1", "c3", "c4", "c5", "c6"])
def test_device_generator_matches_host(zp, cfg):
    n = 3000
    a, o, l_ = zp.batch.generate(cfg, n, first=5, device=dev())
    ha, ho, hl = zp.batch.generate_host(cfg, n, first=5)
    assert (l_.cpu().numpy().astype(np.uint32) == hl).all()
    assert a.cpu().numpy()[:int(ho[-1] + hl[-1])].tobytes() == ha[:int(ho[-1] + hl[-1])].tobytes()


# ---- fuzz & layouts -------------------------------------------------------

def fuzz_frames(zp, golden, count, seed, repair_p=0.0):
    """Mutated golden and generated frames; with repair_p, that share of them
    gets its checksums refilled (tests/fuzzfix.py) so it reaches the checks
    after the checksums and the accept path."""
    from fuzzfix import repair
    rng = random.Random(seed)
    seeds = [bytes.fromhex(fx["bytes"]) for fx in golden["fixtures"]]
    for cfg in ("c3", "c4", "c5") + (("c1", "c6") if repair_p else ()):
        a, o, l_ = zp.batch.generate_host(cfg, 64, first=seed)
        seeds += [a[x:x + y].tobytes() for x, y in zip(o, l_)]
    out = []
    for _ in range(count):
        f = rng.choice(seeds)
        for _ in range(rng.randint(0, 2)):
            f = mutate(rng, f)
        if repair_p and rng.random() < repair_p:
            f = repair(f)
        out.append(f)
    return out


def test_fuzz_gpu_vs_oracle(zp, golden):
    frames = fuzz_frames(zp, golden, 60000, 7)
    arena, offs, lens = pack(frames)
    got, gext = gpu_parse(zp, arena, offs, lens, base_shift=5)
    want, wext = orc.parse_batch(arena, offs, lens)
    assert_same(got, gext, want, wext)
    assert len(np.unique(want["err"])) >= 18


def test_fuzz_repaired_gpu_vs_oracle(zp, golden):
    """Mutations with refilled checksums: most frames pass the checksums, so
    the straight-line IPv4 path, the general walk's field checks and the
    accept path all see mutated headers."""
    frames = fuzz_frames(zp, golden, 60000, 11, repair_p=0.7)
    arena, offs, lens = pack(frames)
    want, wext = orc.parse_batch(arena, offs, lens)
    assert (want["err"] == 0).mean() > 0.4
    for shift in (0, 3):
        got, gext = gpu_parse(zp, arena, offs, lens, base_shift=shift)
        assert_same(got, gext, want, wext)


def test_min_size_tiles_repaired(zp):
    """The register path for tiles of 64-B frames against mutated frames that
    still carry valid checksums: one or two frames per tile get a header or
    L4 byte changed (bytes 12-63, length kept) and their checksums refilled.
    A tile is accepted on the register path only if every frame passes its
    checks; otherwise the whole tile takes the stream path. Both must match
    the oracle, and both must occur."""
    from fuzzfix import repair
    n = 64 * 400
    arena, offs, lens = zp.batch.generate("c1", n, first=4242, device=dev())
    a = arena.cpu().numpy().copy()
    o = offs.cpu().numpy().astype(np.int64)
    rng = random.Random(17)
    for t in range(n // 64):
        for _ in range(rng.randint(1, 2)):
            i = 64 * t + rng.randrange(64)
            f = bytearray(a[o[i]:o[i] + 64].tobytes())
            f[rng.randrange(12, 64)] = rng.choice([0, 1, 2, 4, 5, 6, 15, 16, 17, 0x40, 0x45,
                                                   0x46, 0x50, 0xF0, 255, rng.randrange(256)])
            if rng.random() < 0.85:
                f = repair(bytes(f))
            a[o[i]:o[i] + 64] = np.frombuffer(bytes(f), np.uint8)
    lens_np = lens.cpu().numpy()
    want, wext = orc.parse_batch(a, o.astype(np.uint64), lens_np)
    ok_tiles = (want["err"].reshape(-1, 64) == 0).all(1).mean()
    assert 0.2 < ok_tiles < 0.9, ok_tiles
    for shift in (0, 2, 5, 12):
        got, gext = gpu_parse(zp, a, o, lens_np, base_shift=shift)
        assert_same(got, gext, want, wext)
    # the field checks around the checksums are reached: IPv4 version, total
    # length, TCP data offset, UDP length
    assert {9, 12, 26, 29} <= set(np.unique(want["err"]).tolist())


LAYOUTS = ["shuffled", "gaps", "overlap", "reverse", "dup"]


def layout_batch(frames, layout):
    """frames -> (arena, offs, lens) with the descriptors in one of LAYOUTS."""
    arena, offs, lens = pack(frames, base_pad=3, gap=(13 if layout == "gaps" else 0))
    rng = np.random.default_rng(3)
    if layout == "shuffled":
        p = rng.permutation(len(offs))
        offs, lens = offs[p], lens[p]
    elif layout == "reverse":
        offs, lens = offs[::-1].copy(), lens[::-1].copy()
    elif layout == "overlap":
        # frames that share bytes: a second view starting 7 bytes into each frame
        offs = np.concatenate([offs, offs + 7]).astype(np.uint64)
        lens = np.concatenate([lens, np.maximum(lens.astype(np.int64) - 7, 0)]).astype(np.uint32)
    elif layout == "dup":
        idx = rng.integers(0, len(offs), 8000)
        offs, lens = offs[idx], lens[idx]
    return arena, offs, lens


@pytest.mark.parametrize("layout", LAYOUTS)
def test_layouts(zp, golden, layout):
    frames = fuzz_frames(zp, golden, 5000, 11)
    arena, offs, lens = layout_batch(frames, layout)
    got, gext = gpu_parse(zp, arena, offs, lens)
    want, wext = orc.parse_batch(arena, offs, lens)
    assert_same(got, gext, want, wext)


def test_frames_far_apart_in_one_tile(zp, golden):
    """Frames of one tile 17 GiB apart: the stream's per-frame 64-bit chunk
    origins (a tile is not a contiguous region). A 17 GiB arena with the
    frames of every other tile split between its two ends, alternating
    within the tile."""
    frames = fuzz_frames(zp, golden, 512, 29, repair_p=0.5)
    gap = 17 << 30
    d = dev()
    arena = torch.zeros(gap + (1 << 20), dtype=torch.uint8, device=d)
    lo = hi = 0
    offs = []
    for i, f in enumerate(frames):
        tile_split = (i // 64) % 2 == 1
        if tile_split and i % 2:
            offs.append(gap + hi); hi += len(f) + 1
        else:
            offs.append(lo); lo += len(f) + 1
    assert lo < gap and hi < (1 << 20)
    for o, f in zip(offs, frames):
        if f:
            arena[o:o + len(f)] = torch.frombuffer(bytearray(f), dtype=torch.uint8).to(d)
    offs_t = torch.tensor(offs, dtype=torch.int64, device=d)
    lens_t = torch.tensor([len(f) for f in frames], dtype=torch.int32, device=d)
    r, e = zp.batch.parse_batch(arena, offs_t, lens_t)
    torch.cuda.synchronize()
    got, gext = zp.batch.records_to_numpy(r, e)
    del arena
    torch.cuda.empty_cache()
    a, o, l_ = pack(frames)
    want, wext = orc.parse_batch(a, o, l_)
    assert_same(got, gext, want, wext)
    assert (want["err"] == 0).sum() > 100


def test_edge_lengths_and_empty(zp):
    d = dev()
    # n == 0: no launch, no error
    a = torch.zeros(64, dtype=torch.uint8, device=d)
    r, e = zp.batch.parse_batch(a, torch.zeros(0, dtype=torch.int64, device=d),
                                torch.zeros(0, dtype=torch.int32, device=d))
    assert r.numel() == 0
    # every length 0..200 of a valid frame, the last one ending at the arena end
    ha, ho, hl = zp.batch.generate_host("c3", 1, first=42)
    base = ha[int(ho[0]):int(ho[0] + hl[0])].tobytes()
    frames = [base[:k] for k in range(0, min(len(base), 200) + 1)]
    arena, offs, lens = pack(frames)
    arena = arena[:int(offs[-1] + lens[-1])]            # tight arena end
    got, gext = gpu_parse(zp, arena, offs, lens)
    want, wext = orc.parse_batch(arena, offs, lens)
    assert_same(got, gext, want, wext)


def _jumbo_ipv6(total_len, rng, valid=True, proto=17, fill=None):
    """IPv6 UDP/ICMPv6 frame of total_len bytes (payload_length is never
    checked by the parser, so frames > 64 KiB are legal input); fill: a
    constant byte instead of random bytes."""
    from pybuilder import internet_checksum, pseudo_header
    f = bytearray(rng.integers(0, 256, total_len, dtype=np.uint8).tobytes() if fill is None
                  else bytes([fill]) * total_len)
    f[12:14] = b"\x86\xdd"
    f[14] = 0x60
    f[20] = proto
    seg = total_len - 54
    if proto == 17:
        f[54 + 4:54 + 6] = (seg & 0xFFFF).to_bytes(2, "big")
        f[58:60] = b"\0\0"
        c = internet_checksum(f[54:], pseudo_header(f[22:38], f[38:54], 17, seg))
        f[60:62] = (c if valid else c ^ 0x1).to_bytes(2, "big")
    else:
        f[54] = 128
        f[56:58] = b"\0\0"
        c = internet_checksum(f[54:], pseudo_header(f[22:38], f[38:54], 58, seg))
        f[56:58] = (c if valid else c ^ 0x1).to_bytes(2, "big")
    return bytes(f)


def jumbo_frames():
    """65,535-300,000 B, UDP and ICMPv6, valid and corrupt checksums."""
    rng = np.random.default_rng(5)
    frames = []
    for L in (65535, 65600, 70001, 140000, 200003, 300000):
        for proto in (17, 58):
            frames.append(_jumbo_ipv6(L, rng, True, proto))
            frames.append(_jumbo_ipv6(L, rng, False, proto))
    return frames


def word_sum_frames():
    """65,534-65,537 B of 0xFF, valid and corrupt ICMPv6 checksums in turn."""
    rng = np.random.default_rng(9)
    return [_jumbo_ipv6(L, rng, ok, 58, fill=0xFF)
            for L in (65534, 65535, 65536, 65537) for ok in (True, False)]


def test_jumbo_frames_exact_path(zp):
    """Segments > 64 KiB take the exact E/O path (u32 wrap reproduced)."""
    frames = jumbo_frames()
    arena, offs, lens = pack(frames)
    got, gext = gpu_parse(zp, arena, offs, lens, base_shift=1)
    want, wext = orc.parse_batch(arena, offs, lens)
    assert_same(got, gext, want, wext)
    # UDP length field wraps for > 64 KiB segments -> UDP_LENGTH; ICMPv6 hits the checksum
    assert set(np.unique(want["err"])) >= {0, ERR["IPV6_L4_CHECKSUM"]}


def test_word_sum_bounds(zp):
    """The largest frames of the stream path (65,536 B) and the first of the
    exact path (65,537 B), all-0xFF payloads (the largest word sums the u32
    stream arithmetic meets), valid and corrupt ICMPv6 checksums, at both
    arena parities."""
    frames = word_sum_frames()
    arena, offs, lens = pack(frames)
    want, wext = orc.parse_batch(arena, offs, lens)
    assert list(want["err"][0::2]) == [0, 0, 0, 0]
    for shift in (0, 1):
        got, gext = gpu_parse(zp, arena, offs, lens, base_shift=shift)
        assert_same(got, gext, want, wext)


def test_all_zero_icmp_never_valid(zp):
    """S == 0 (acc 0, all-zero ICMPv4 message) is invalid (checksum.rs:28)."""
    from pybuilder import Builder
    ip1, ip2 = [10, 0, 0, 1], [10, 0, 0, 2]
    f = bytearray(Builder(98).ethernet([1] * 6, [2] * 6, 0x0800)
                  .ipv4(4, 5, 0, 0, 84, 0, 0, 0, 64, 1, ip1, ip2).icmpv4(0, 0).build())
    f[36:] = bytes(len(f) - 36)            # ICMP type 0 code 0 checksum 0, zero body
    arena, offs, lens = pack([bytes(f)])
    got, gext = gpu_parse(zp, arena, offs, lens)
    want, wext = orc.parse_batch(arena, offs, lens)
    assert want["err"][0] == ERR["IPV4_L4_CHECKSUM"]
    assert_same(got, gext, want, wext)


# ---- host-buffer path -------------------------------------------------------

@pytest.mark.parametrize("pinned", [False, True])
def test_host_path(zp, golden, pinned):
    frames = fuzz_frames(zp, golden, 20000, 21)
    arena, offs, lens = pack(frames)
    if pinned:
        t = torch.from_numpy(arena).pin_memory()
        arena = t.numpy()
    lib = zp._lib.hip()
    ctx = lib.zp_ctx_create(0, 1 << 20)           # small chunks: many slots in flight
    assert ctx
    rec = np.zeros(len(offs), zp.records.RECORD_DTYPE)
    ext = np.zeros((2, len(offs)), zp.records.EXT_DTYPE)
    rc = lib.zp_parse_batch_host(ctx, arena.ctypes.data, len(arena), offs.ctypes.data,
                                 lens.ctypes.data, len(offs), rec.ctypes.data, ext.ctypes.data)
    lib.zp_ctx_destroy(ctx)
    assert rc == 0, lib.zp_last_error()
    want, wext = orc.parse_batch(arena, offs, lens)
    assert_same(rec, ext, want, wext)


def test_host_path_multi(zp, golden):
    """zp_parse_batch_host_multi: byte-balanced ranges over several contexts
    (here 3 contexts sharing device 0), concurrently, results in place."""
    frames = fuzz_frames(zp, golden, 15000, 23)
    arena, offs, lens = pack(frames)
    lib = zp._lib.hip()
    ctxs = [lib.zp_ctx_create(0, 1 << 20) for _ in range(3)]
    assert all(ctxs)
    arr = (ctypes.c_void_p * 3)(*ctxs)
    rec = np.zeros(len(offs), zp.records.RECORD_DTYPE)
    ext = np.zeros((2, len(offs)), zp.records.EXT_DTYPE)
    rc = lib.zp_parse_batch_host_multi(arr, 3, arena.ctypes.data, len(arena), offs.ctypes.data,
                                       lens.ctypes.data, len(offs), rec.ctypes.data,
                                       ext.ctypes.data)
    for c in ctxs:
        lib.zp_ctx_destroy(c)
    assert rc == 0, lib.zp_last_error()
    want, wext = orc.parse_batch(arena, offs, lens)
    assert_same(rec, ext, want, wext)


# ---- full-size properties (BASELINE configs 3-5) ----------------------------

@pytest.mark.parametrize("config,n", [("c3", 16 << 20), ("c4", 16 << 20), ("c5", 32 << 20),
                                      ("c6", 16 << 20)])
def test_full_size_properties(zp, config, n):
    """BASELINE configs 3-5 at full per-GPU size (c3/c4: 16M frames; c5: one
    GPU's shard of the 256M IMIX = 32M frames) and the mixed config c6:
    every frame accepted, a random sample byte-exact vs the oracle, idempotent
    re-parse, and flipping one bit of every frame's last byte turns every
    record into the L4 checksum error of its innermost IP version (ARP frames,
    which carry no checksum, stay accepted and unchanged)."""
    from importlib import import_module
    rec = import_module("zero-packet_amd.records")
    arena, offs, lens = zp.batch.generate(config, n, device=dev())
    zeros = lambda: torch.zeros((2, n, 16), dtype=torch.uint8, device=arena.device)
    r1, e1 = zp.batch.parse_batch(arena, offs, lens, ext=zeros())
    assert int((zp.batch.record_err(r1) != 0).sum()) == 0
    r2, e2 = zp.batch.parse_batch(arena, offs, lens, ext=zeros())
    assert torch.equal(r1, r2) and torch.equal(e1, e2)
    idx = torch.randint(0, n, (2000,), device=arena.device, generator=torch.Generator(
        device=arena.device).manual_seed(1))
    so, sl = offs[idx].cpu().numpy(), lens[idx].cpu().numpy()
    frames = [arena[int(o):int(o) + int(l)].cpu().numpy() for o, l in zip(so, sl)]
    sa, sof, sle = pack([f.tobytes() for f in frames])
    want, wext = orc.parse_batch(sa, sof, sle)
    got, gext = zp.batch.records_to_numpy(r1[idx], e1[:, idx])
    assert_same(got, gext, want, wext)
    flags = zp.batch.record_flags(r1)
    ipip = (flags & rec.F_IP_IN_IP) != 0
    v6 = torch.where(ipip, (flags & rec.F_IP_IN_IP_V6) != 0, (flags & rec.F_IPV6) != 0)
    want_err = torch.where(v6, ERR["IPV6_L4_CHECKSUM"], ERR["IPV4_L4_CHECKSUM"]).to(torch.uint8)
    arp = (flags & rec.F_ARP) != 0
    want_err[arp] = 0
    del r2, e2
    last = offs + lens.to(torch.int64) - 1
    arena[last] ^= 1
    r3, _ = zp.batch.parse_batch(arena, offs, lens)
    torch.cuda.synchronize()
    assert torch.equal(zp.batch.record_err(r3), want_err)
    assert torch.equal(r3[arp], r1[arp])


# ---- maximum size: the whole BASELINE config 5 on one GPU ------------------

def test_max_size_full_imix_one_gpu(zp):
    """All 268,435,456 IMIX frames of config 5 (95 GB, arena offsets past
    2^36, 4M workgroups) in one launch: every frame accepted, 4,000 sampled
    frames (the last 1,000 among them) byte-exact vs the oracle."""
    torch.cuda.empty_cache()                 # earlier tests' cached blocks
    free, _ = torch.cuda.mem_get_info()
    if free < 120e9:
        pytest.skip(f"needs ~110 GB of free HBM, {free / 1e9:.0f} GB free")
    n = 256 << 20
    arena, offs, lens = zp.batch.generate("c5", n, device=dev())
    assert int(offs[-1].item()) > (1 << 36)
    rec, ext = zp.batch.parse_batch(arena, offs, lens)
    assert int((zp.batch.record_err(rec) != 0).sum()) == 0
    g = torch.Generator(device=arena.device).manual_seed(5)
    idx = torch.cat([torch.randint(0, n, (3000,), device=arena.device, generator=g),
                     torch.arange(n - 1000, n, device=arena.device)])
    so, sl = offs[idx].cpu().numpy(), lens[idx].cpu().numpy()
    frames = [arena[int(o):int(o) + int(l)].cpu().numpy().tobytes() for o, l in zip(so, sl)]
    del arena
    sa, sof, sle = pack(frames)
    want, wext = orc.parse_batch(sa, sof, sle)
    got, gext = zp.batch.records_to_numpy(rec[idx], ext[:, idx])
    assert_same(got, gext, want, wext)


# ---- API guards ------------------------------------------------------------

def test_descriptor_bounds_refused(zp):
    """Frames past the arena, negative offsets/lengths and mis-shaped outputs
    are refused before any launch (the kernel does not check descriptors)."""
    d = dev()
    a = torch.zeros(1024, dtype=torch.uint8, device=d)
    o = torch.tensor([0, 512], dtype=torch.int64, device=d)
    good = torch.tensor([64, 512], dtype=torch.int32, device=d)
    zp.batch.parse_batch(a, o, good)                              # ends exactly at the arena end
    for lens in ([64, 513], [64, -1]):
        with pytest.raises(ValueError):
            zp.batch.parse_batch(a, o, torch.tensor(lens, dtype=torch.int32, device=d))
    with pytest.raises(ValueError):
        zp.batch.parse_batch(a, torch.tensor([0, -64], dtype=torch.int64, device=d), good)
    with pytest.raises(ValueError):
        zp.batch.parse_batch(a, o, good, records=torch.empty((2, 4), dtype=torch.uint8, device=d))
    with pytest.raises(ValueError):
        zp.batch.parse_batch(a, o, good, ext=torch.empty((2, 2, 16), dtype=torch.uint8))
    with pytest.raises(ValueError):
        zp.columns.parse_with_columns(a, o, torch.tensor([64, 600], dtype=torch.int32, device=d))
    r, _ = zp.batch.parse_batch(a, o, good)
    with pytest.raises(ValueError):
        zp.columns.extract(a, o, torch.tensor([2048, 64], dtype=torch.int32, device=d), r)


def test_parse_one_threads(zp, golden):
    """PacketParser.parse from several threads at once (one shared zp_ctx
    behind a lock): every thread gets its own frame's result."""
    import threading
    frames = [bytes.fromhex(fx["bytes"]) for fx in golden["fixtures"]]

    def result(f):
        try:
            return zp.parser.PacketParser.parse(f).debug()
        except zp.parser.ZeroPacketError as e:     # Err(&str): same string each time
            return repr(e)
    want = [result(f) for f in frames]
    bad = []

    def worker(k):
        for it in range(40):
            i = (k + it) % len(frames)
            if result(frames[i]) != want[i]:
                bad.append((k, it, i))
    ts = [threading.Thread(target=worker, args=(k,)) for k in range(8)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not bad, bad[:5]


def test_ext_null_and_sparse(zp, golden):
    """ext = NULL drops the chains only (records identical); with an ext array
    the flagged chains match the oracle both where a wave holds many chains
    (whole-wave writes) and where it holds one (that entry only); a sentinel
    shows which entries a wave leaves untouched. c4's chains are short and in
    RFC order: they go inline in the record (ABI v6) and their entries are
    never written; chains behind an ip_in_ip header (or long / out of order)
    keep their entries."""
    import ctypes
    R = zp.records
    arena, offs, lens = zp.batch.generate("c4", 4096, device=dev())
    ext_rich = torch.full((2, 4096, 16), 0xA5, dtype=torch.uint8, device=dev())
    r1, _ = zp.batch.parse_batch(arena, offs, lens, ext=ext_rich)
    r0 = torch.empty_like(r1)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert zp._lib.hip().zp_parse_batch_device(arena.data_ptr(), offs.data_ptr(), lens.data_ptr(),
                                               4096, r0.data_ptr(), None, s) == 0
    torch.cuda.synchronize()
    assert torch.equal(r0, r1)
    want, wext = orc.parse_batch(arena.cpu().numpy(), offs.cpu().numpy(), lens.cpu().numpy())
    got, gext = zp.batch.records_to_numpy(r1, ext_rich)
    assert_same(got, gext, want, wext)
    inl = R.chain_inline(got)
    chained = (want["flags"] & R.F_EXT) != 0
    assert chained.sum() > 3000 and (inl == chained).all()        # every c4 chain inline
    assert (ext_rich.cpu().numpy()[0][inl] == 0xA5).all()         # ... and no entry written
    # chains that keep their entries: behind ip_in_ip / out of RFC order
    fx = [bytes.fromhex(f["bytes"]) for f in golden["fixtures"]]
    wide = []
    for f in fx:
        err, rec, ext = orc.parse_one(f)
        if not err and int(rec["flags"]) & R.F_EXT and not R.chain_inline(orc.pack(rec, ext))[0]:
            wide.append(f)
    assert wide
    a3, o3, l3 = zp.batch.generate("c3", 127, device=dev())
    c3 = [a3[int(o):int(o) + int(l)].cpu().numpy().tobytes()
          for o, l in zip(o3.cpu().numpy(), l3.cpu().numpy())]
    d = dev()
    for frames, k_rich in (([wide[i % len(wide)] for i in range(128)], True),   # dense wave
                           (c3[:70] + [wide[0]] + c3[70:], False)):            # sparse wave
        a, o, l_ = pack(frames)
        ta = torch.from_numpy(a).to(d)
        to = torch.from_numpy(o.astype(np.int64)).to(d)
        tl = torch.from_numpy(l_.astype(np.int32)).to(d)
        ext = torch.full((2, 128, 16), 0xA5, dtype=torch.uint8, device=d)
        r, _ = zp.batch.parse_batch(ta, to, tl, ext=ext)
        want, wext = orc.parse_batch(a, o, l_)
        got, gext = zp.batch.records_to_numpy(r, ext)
        assert_same(got, gext, want, wext)
        e = ext.cpu().numpy()
        flagged = (want["flags"] & R.F_EXT) != 0
        assert not R.chain_inline(got).any()
        assert (e[0][flagged] != 0xA5).any(axis=1).all()          # written entries
        if not k_rich:
            assert flagged.sum() == 1
            untouched = [i for i in range(128) if i != 70]
            assert (e[0, untouched] == 0xA5).all()


@pytest.mark.parametrize("cfg", ["c1", "c3"])
def test_common_frame_path_mutations(zp, cfg):
    """The straight-line path for Ethernet / IPv4 (20-B header) / TCP, UDP,
    ICMPv4 frames runs when most of a wave has that shape: mutate header and
    payload bytes of a quarter of such frames (every check of the path fails
    somewhere, the rest stay valid) and compare every record with the oracle."""
    arena, offs, lens = zp.batch.generate(cfg, 40000, first=4242, device=dev())
    a = arena.cpu().numpy().copy()
    o, l_ = offs.cpu().numpy(), lens.cpu().numpy()
    rng = np.random.default_rng(11)
    pick = rng.random(len(o)) < 0.25
    for i in np.nonzero(pick)[0]:
        k = int(rng.integers(0, 4))
        if k == 0:                              # a header byte (Ethernet, IPv4, L4 words)
            j = int(rng.choice([12, 13, 14, 16, 17, 22, 23, 24, 25, 34, 35, 38, 39, 46, 47]))
        elif k == 1:                            # any byte of the first 64
            j = int(rng.integers(0, 64))
        else:                                   # any byte (the L4 checksum)
            j = int(rng.integers(0, int(l_[i])))
        a[int(o[i]) + j] ^= np.uint8(1 << int(rng.integers(0, 8)))
    want, wext = orc.parse_batch(a, o, l_)
    assert (want["err"] == 0).sum() > 25000 and (want["err"] != 0).sum() > 5000
    for shift in (0, 3):
        got, gext = gpu_parse(zp, a, o, l_, base_shift=shift)
        assert_same(got, gext, want, wext)


@pytest.mark.parametrize("layout", ["packed", "shuffled"])
def test_min_size_tiles(zp, layout):
    """Tiles whose frames are all 64 B take the register path; one frame of
    another shape, or failing a check, sends its whole tile to the stream
    path. 64-B frames (c1) with a few single-bit flips (header and L4 bytes:
    wrong shapes, failed checks and checksums), a ragged last tile, every
    frame alignment mod 4 (packed at base shifts 0-3, or shuffled offsets
    with gaps), and an ICMP frame whose L4 bytes are all zero."""
    arena, offs, lens = zp.batch.generate("c1", 64 * 300 + 17, first=99, device=dev())
    a = arena.cpu().numpy().copy()
    o, l_ = offs.cpu().numpy().astype(np.int64), lens.cpu().numpy()
    assert (l_ == 64).all()
    rng = np.random.default_rng(5)
    for i in rng.choice(len(o), 60, replace=False):
        j = int(rng.integers(0, 64))
        a[o[i] + j] ^= np.uint8(1 << int(rng.integers(0, 8)))
    frames = [a[x:x + 64].tobytes() for x in o]
    want_n = None
    if layout == "packed":
        pa, po, pl = pack(frames)
        want, wext = orc.parse_batch(pa, po, pl)
        want_n = int((want["err"] != 0).sum())
        for shift in (0, 1, 2, 3, 4, 7, 8, 13, 15):   # every dword offset in a 16-B chunk
            got, gext = gpu_parse(zp, pa, po, pl, base_shift=shift)
            assert_same(got, gext, want, wext)
    else:
        order = rng.permutation(len(frames))
        pos, po = 0, np.zeros(len(frames), np.int64)
        for k in order:
            pos += int(rng.integers(0, 20))
            po[k] = pos
            pos += 64
        pa = np.zeros(pos + 64, np.uint8)
        for k, f in enumerate(frames):
            pa[po[k]:po[k] + 64] = np.frombuffer(f, np.uint8)
        pl = np.full(len(frames), 64, np.uint32)
        want, wext = orc.parse_batch(pa, po.astype(np.uint64), pl)
        want_n = int((want["err"] != 0).sum())
        got, gext = gpu_parse(zp, pa, po, pl)
        assert_same(got, gext, want, wext)
    assert 10 <= want_n <= 60


def test_min_size_tiles_small_batches(zp):
    """The register path at batch edges: 1, 5, 64 and 65 frames of 64 B, and a
    tile whose 64 descriptors all name the same frame."""
    arena, offs, lens = zp.batch.generate("c1", 65, first=7, device=dev())
    a, o, l_ = arena.cpu().numpy(), offs.cpu().numpy(), lens.cpu().numpy()
    for n in (1, 5, 63, 64, 65):
        want, wext = orc.parse_batch(a, o[:n], l_[:n])
        for shift in (0, 1, 6, 11):
            got, gext = gpu_parse(zp, a, o[:n], l_[:n], base_shift=shift)
            assert_same(got, gext, want, wext)
    same = np.full(64, o[3], np.uint64)
    want, wext = orc.parse_batch(a, same, l_[:64])
    got, gext = gpu_parse(zp, a, same, l_[:64])
    assert_same(got, gext, want, wext)
    assert (want["err"] == 0).all()


def test_config2_full_batch_exact(zp):
    """BASELINE config 2 in full: the 1M x 64-B Eth+IPv4+UDP batch on the GPU,
    byte-for-byte against the CPU oracle on the same frames (config 1)."""
    import torch
    arena, offs, lens = zp.batch.generate("c2", 1 << 20, device=dev())
    recs, ext = zp.batch.parse_batch(arena, offs, lens)
    torch.cuda.synchronize()
    got, gext = zp.batch.records_to_numpy(recs, ext)
    want, wext = orc.parse_batch(arena.cpu().numpy(), offs.cpu().numpy(), lens.cpu().numpy())
    assert (want["err"] == 0).all() and (lens.cpu().numpy() == 64).all()
    assert got.tobytes() == orc.pack(want, wext).tobytes()
    assert zp.records.ext_match(gext, wext, want)


def _fast_ip_probe(f):
    """zp_parse.hip fast_ip_probe in Python: the frames a wave may take the
    mixed-stack straight-line path for (every frame of a wave must pass)."""
    if len(f) < 64:
        return False
    t0 = (f[12] << 8) | f[13]
    hl = 18 if t0 == 0x8100 else (22 if t0 == 0x88A8 else 14)
    et = (f[hl - 2] << 8) | f[hl - 1]
    if et == 0x0800:
        return f[hl] == 0x45
    return et == 0x86DD and f[hl + 6] not in (0, 43, 44, 51, 60)


def test_mixed_stack_path_mutations(zp):
    """The straight-line path for mixed stacks (fast_ip: 0/1/2 tags, IPv4
    without options or IPv6 without extensions, one IP-in-IP level, every L4
    reader) on c5 frames with header bytes mutated (tags, ethertypes,
    versions, lengths, protocols at both levels, L4 fields), half of them
    with their checksums refilled so the checks after the checksums and the
    accept path see unusual values; only frames that pass the path's wave
    probe are kept, so whole waves take it. Every record equals the oracle's."""
    from fuzzfix import repair
    rng = random.Random(5)
    a, o, l_ = zp.batch.generate_host("c5", 70000, first=31337)
    frames = []
    vals = [0, 1, 4, 6, 17, 41, 43, 44, 51, 58, 59, 60, 0x45, 0x46, 0x40, 0x60, 0x65, 0x81, 0x00,
            0x86, 0xdd, 0x88, 0xa8, 0x08, 0xff, 5, 8, 128, 135]
    for x, y in zip(o, l_):
        f = bytearray(a[int(x):int(x) + int(y)].tobytes())
        if rng.random() < 0.4:
            for _ in range(rng.randint(1, 2)):
                j = rng.randrange(12, min(len(f), 120))
                f[j] = rng.choice(vals) if rng.random() < 0.6 else rng.randrange(256)
            if rng.random() < 0.5:
                f = bytearray(repair(bytes(f)))
        f = bytes(f)
        if _fast_ip_probe(f):
            frames.append(f)
    arena, offs, lens = pack(frames)
    want, wext = orc.parse_batch(arena, offs, lens)
    nerr = int((want["err"] != 0).sum())
    assert len(frames) > 60000 and nerr > 5000 and len(frames) - nerr > 40000
    assert len(set(want["err"].tolist())) >= 12
    # accepted frames of every stack the path takes: tags, both versions,
    # IP-in-IP of both inner versions, the four L4 readers
    ok = want[want["err"] == 0]
    F = zp.records
    for bit in (F.F_IPV4, F.F_IPV6, F.F_IP_IN_IP, F.F_IP_IN_IP_V6, F.F_TCP, F.F_UDP, F.F_ICMPV4,
                F.F_ICMPV6):
        assert ((ok["flags"] & bit) != 0).sum() > 100, bit
    assert len(set(ok["eth_len"].tolist())) == 3
    for shift in (0, 5):
        got, gext = gpu_parse(zp, arena, offs, lens, base_shift=shift)
        assert_same(got, gext, want, wext)


def test_parse_one_sizes(zp):
    """zp_parse_one on both of its paths: frames up to 64 KiB through the
    mapped block (the resident server wave, then one batch launch per call,
    read the frame and write the record over the host link), longer ones
    through the batch host path; records and chains equal the oracle's,
    unflagged chain entries zero."""
    import ctypes
    rng = np.random.default_rng(13)
    a, o, l_ = zp.batch.generate_host("c4", 40, first=77)
    frames = [a[int(x):int(x) + int(y)].tobytes() for x, y in zip(o, l_)]
    frames += [_jumbo_ipv6(L, rng, ok, p) for L in (65535, 65536, 65537, 90000)
               for ok in (True, False) for p in (17, 58)]
    frames += [b"", b"\x00" * 63]
    lib = zp._lib.hip()
    ctx = lib.zp_ctx_create(0, 0)
    try:
        for idle in (5000, 0):
            assert lib.zp_parse_one_config(ctx, idle) == 0
            for f in frames:
                rec = np.zeros(1, zp.records.RECORD_DTYPE)
                ext = np.full((2, 16), 0xA5, np.uint8)
                buf = ctypes.create_string_buffer(f, max(len(f), 1))
                rc = lib.zp_parse_one(ctx, ctypes.addressof(buf), len(f), rec.ctypes.data,
                                      ext.ctypes.data)
                err, wrec, wext = orc.parse_one(f)
                assert rc == err and rec.tobytes() == orc.pack(wrec, wext).tobytes(), \
                    (idle, len(f), rc, err)
                assert ext.tobytes() == wext.view(np.uint8).tobytes(), (idle, len(f))
    finally:
        lib.zp_ctx_destroy(ctx)


def _v6_in_v6(outer_hbh, inner_hbh, l4="udp", tail=40, seed=0, valid=True):
    """Ethernet + IPv6 (+ a 16-B Hop-by-Hop header) + IPv6 (+ a 16-B
    Hop-by-Hop header) + UDP / ICMPv6 with its checksum over the inner
    pseudo-header: the outer chain sits in front of an ip_in_ip header and
    the inner one is an inner chain, so both keep their entries (ABI v6)."""
    from pybuilder import internet_checksum, pseudo_header
    rng = np.random.default_rng(seed)
    proto = {"udp": 17, "icmpv6": 58}[l4]
    f = bytearray(rng.integers(0, 256, 14 + 80 + 16 * (outer_hbh + inner_hbh) + tail,
                               dtype=np.uint8).tobytes())
    f[12:14] = b"\x86\xdd"
    pos = 14
    for k, hbh in enumerate((outer_hbh, inner_hbh)):
        nxt = 41 if k == 0 else proto
        f[pos] = 0x60
        if hbh:
            f[pos + 6] = 0                                  # Hop-by-Hop (headers.rs:90-113)
            f[pos + 40] = nxt
            f[pos + 41] = 1                                 # (1 + 1) * 8 = 16 B
        else:
            f[pos + 6] = nxt
        ip = pos
        pos += 40 + 16 * hbh
    src, dst = f[ip + 8:ip + 24], f[ip + 24:ip + 40]
    if l4 == "udp":
        f[pos + 4:pos + 6] = tail.to_bytes(2, "big")        # length == slice (parser.rs:262)
        ck = pos + 6
    else:
        f[pos] = 128                                        # echo request
        ck = pos + 2
    f[ck:ck + 2] = b"\0\0"
    c = internet_checksum(f[pos:], pseudo_header(src, dst, proto, tail))
    f[ck:ck + 2] = (c if valid else c ^ 0x0101).to_bytes(2, "big")
    return bytes(f)


def test_parse_one_chain_entries(zp):
    """zp_parse_one on frames whose chains keep their entries (an outer chain
    in front of ip_in_ip, an inner chain): the server stores the entries,
    waits for them, then the record with its acknowledgement in one 16-B
    store; both modes equal the oracle, entries included."""
    import ctypes
    R = zp.records
    frames = [_v6_in_v6(o, i, l4, seed=s, valid=v)
              for o in (0, 1) for i in (0, 1) for l4 in ("udp", "icmpv6")
              for s, v in ((1, True), (2, False), (3, True))]
    want = [orc.parse_one(f) for f in frames]
    flags = [int(w[1]["flags"]) for w in want if w[0] == 0]
    assert any(x & R.F_INNER_EXT for x in flags) and any(x & R.F_EXT for x in flags)
    assert sum(1 for w in want if w[0]) >= 8
    lib = zp._lib.hip()
    ctx = lib.zp_ctx_create(0, 0)
    try:
        for idle in (5000, 0, 5000):
            assert lib.zp_parse_one_config(ctx, idle) == 0
            for rep in range(3):
                for f, (err, wrec, wext) in zip(frames, want):
                    rec = np.zeros(1, R.RECORD_DTYPE)
                    ext = np.full((2, 16), 0xA5, np.uint8)
                    buf = ctypes.create_string_buffer(f, len(f))
                    rc = lib.zp_parse_one(ctx, ctypes.addressof(buf), len(f), rec.ctypes.data,
                                          ext.ctypes.data)
                    assert rc == err and rec.tobytes() == orc.pack(wrec, wext).tobytes(), \
                        (idle, rep, len(f), rc, err)
                    assert ext.tobytes() == wext.view(np.uint8).tobytes(), (idle, rep, len(f))
    finally:
        lib.zp_ctx_destroy(ctx)


def _udp4(total, seed, valid=True):
    """Ethernet + IPv4 (IHL 5) + UDP frame of `total` bytes, checksums valid
    (or the UDP one off by one bit pair)."""
    from pybuilder import internet_checksum, pseudo_header
    rng = np.random.default_rng(seed)
    f = bytearray(rng.integers(0, 256, total, dtype=np.uint8).tobytes())
    f[12:14] = b"\x08\x00"
    f[14:16] = b"\x45\x00"
    f[16:18] = (total - 14).to_bytes(2, "big")
    f[20:22] = b"\0\0"
    f[23] = 17
    f[24:26] = b"\0\0"
    f[24:26] = internet_checksum(f[14:34]).to_bytes(2, "big")
    f[38:40] = (total - 34).to_bytes(2, "big")
    f[40:42] = b"\0\0"
    c = internet_checksum(f[34:], pseudo_header(f[26:30], f[30:34], 17, total - 34))
    f[40:42] = (c if valid else c ^ 0x0101).to_bytes(2, "big")
    return bytes(f)


def test_parse_one_lengths(zp):
    """zp_parse_one at every length from 1,490 to 1,540 bytes (around the
    Ethernet maximum) and at short ones, accepted and rejected, back to back
    so that each request overwrites the previous one's bytes in the block;
    both modes equal the oracle."""
    import ctypes
    R = zp.records
    frames = [_udp4(L, L, valid=(L % 3 != 0)) for L in range(1490, 1541)]
    frames += [_udp4(L, L) for L in (64, 65, 75, 76, 77, 100, 111, 112, 113, 127, 128, 129)]
    frames += [bytes(f[:L]) for f, L in ((_udp4(200, 1), 40), (_udp4(200, 2), 63))]
    want = [orc.parse_one(f) for f in frames]
    assert sum(1 for w in want if w[0] == 0) > 30 and sum(1 for w in want if w[0]) > 15
    lib = zp._lib.hip()
    ctx = lib.zp_ctx_create(0, 0)
    rng = np.random.default_rng(3)
    try:
        for idle in (5000, 0):
            assert lib.zp_parse_one_config(ctx, idle) == 0
            for i in list(range(len(frames))) + list(rng.integers(0, len(frames), 300)):
                f, (err, wrec, wext) = frames[i], want[i]
                rec = np.zeros(1, R.RECORD_DTYPE)
                ext = np.full((2, 16), 0xA5, np.uint8)
                buf = ctypes.create_string_buffer(f, max(len(f), 1))
                rc = lib.zp_parse_one(ctx, ctypes.addressof(buf), len(f), rec.ctypes.data,
                                      ext.ctypes.data)
                assert rc == err and rec.tobytes() == orc.pack(wrec, wext).tobytes(), \
                    (idle, len(f), rc, err)
                assert ext.tobytes() == wext.view(np.uint8).tobytes(), (idle, len(f))
    finally:
        lib.zp_ctx_destroy(ctx)


def test_parse_one_quiesce(zp, golden):
    """PacketParser.parse through the default context's server, quiesce()
    stopping it (the stream of the server wave is then idle, so a device-wide
    synchronisation returns at once), and the next parse relaunching it; the
    results equal the oracle's before and after."""
    import time
    import torch
    frames = [bytes.fromhex(fx["bytes"]) for fx in golden["fixtures"]]

    def result(f):
        try:
            return zp.parser.PacketParser.parse(f).debug()
        except zp.parser.ZeroPacketError as e:
            return repr(e)
    want = [result(f) for f in frames]
    for rep in range(3):
        zp.parser.quiesce()
        t0 = time.perf_counter()
        torch.cuda.synchronize()
        assert time.perf_counter() - t0 < 0.5
        assert [result(f) for f in frames] == want, rep


def test_parse_one_server_lifecycle(zp, golden):
    """The resident zp_parse_one server across its life cycle: a tiny idle
    timeout with random gaps between calls, so that the wave leaves between
    requests, is relaunched by the next call, and sometimes leaves just as a
    doorbell is rung (the host's stream check then relaunches it); stops and
    mode switches in between. Every answer equals the oracle's on accepted
    and rejected frames of every stack (c5, c4, c3, golden, mutated)."""
    import ctypes
    import time
    rng = np.random.default_rng(29)
    frames = [bytes.fromhex(fx["bytes"]) for fx in golden["fixtures"]]
    for cfg, n in (("c5", 300), ("c4", 150), ("c3", 100)):
        a, o, l_ = zp.batch.generate_host(cfg, n, first=5)
        frames += [a[int(x):int(x) + int(y)].tobytes() for x, y in zip(o, l_)]
    mut = []
    for f in frames[:400]:
        b = bytearray(f)
        for _ in range(int(rng.integers(1, 3))):
            b[int(rng.integers(0, min(len(b), 96)))] ^= 1 << int(rng.integers(0, 8))
        mut.append(bytes(b))
    frames += mut
    want = [orc.parse_one(f) for f in frames]
    assert sum(1 for w in want if w[0]) > 100 and sum(1 for w in want if not w[0]) > 400
    lib = zp._lib.hip()
    ctx = lib.zp_ctx_create(0, 0)
    rec = np.zeros(1, zp.records.RECORD_DTYPE)
    ext = np.zeros((2, 16), np.uint8)
    try:
        order = rng.permutation(len(frames))
        for k, i in enumerate(order):
            if k % 250 == 0:                              # mode switches / stops
                lib.zp_parse_one_config(ctx, [40, 0, 2000, 40][(k // 250) % 4])
            f = frames[i]
            buf = ctypes.create_string_buffer(f, max(len(f), 1))
            rc = lib.zp_parse_one(ctx, ctypes.addressof(buf), len(f), rec.ctypes.data,
                                  ext.ctypes.data)
            err, wrec, wext = want[i]
            assert rc == err and rec.tobytes() == orc.pack(wrec, wext).tobytes(), (k, int(i), rc)
            assert ext.tobytes() == wext.view(np.uint8).tobytes(), (k, int(i))
            gap = rng.choice([0.0, 0.0, 20e-6, 45e-6, 200e-6])   # around the 40-us timeout
            if gap:
                time.sleep(gap)
    finally:
        lib.zp_ctx_destroy(ctx)


def _c5_frames(zp, n, seed=5):
    a, o, l_ = zp.batch.generate_host("c5", n, first=seed)
    return [a[int(x):int(x) + int(y)].tobytes() for x, y in zip(o, l_)]


def test_parse_one_sync_bound_under_traffic(zp):
    """A thread calls zp_parse_one back to back (one call every ~10-20 us)
    for 2 s while the main thread times 20 torch.cuda.synchronize() calls:
    the server leaves after its 1 ms life whatever the traffic (the host
    queues the next wave behind it), so no synchronisation waits longer than
    that bound + 1 ms. Control: with a 20 ms life (test hook) a
    synchronisation right after a call waits for the live server, so the
    test sees it. Every answer
    equals the oracle's. The GIL switch interval is lowered to 50 us for the
    test: at Python's 5 ms default, handing the GIL back and forth to the
    calling thread alone costs the timed thread ~10 ms."""
    import sys
    import threading
    import time
    R = zp.records
    frames = _c5_frames(zp, 256)
    want = [orc.parse_one(f) for f in frames]
    bufs = [ctypes.create_string_buffer(f, max(len(f), 1)) for f in frames]
    lib = zp._lib.hip()
    ctx = lib.zp_ctx_create(0, 1 << 20)
    assert ctx
    old_si = sys.getswitchinterval()

    def run(life_us):
        assert lib.zp__one_test_hooks(ctx, life_us, 0, 0) == 0
        stop = threading.Event()
        bad, calls = [], [0]

        def caller():
            rec = np.zeros(1, R.RECORD_DTYPE)
            ext = np.zeros((2, 16), np.uint8)
            k = 0
            while not stop.is_set():
                i = k % len(frames)
                rc = lib.zp_parse_one(ctx, ctypes.addressof(bufs[i]), len(frames[i]),
                                      rec.ctypes.data, ext.ctypes.data)
                err, wrec, wext = want[i]
                if rc != err or rec.tobytes() != orc.pack(wrec, wext).tobytes() \
                        or ext.tobytes() != wext.view(np.uint8).tobytes():
                    bad.append((k, i, rc, err))
                k += 1
            calls[0] = k

        th = threading.Thread(target=caller)
        th.start()
        try:
            time.sleep(0.1)                               # traffic is steady
            waits = []
            t_end = time.perf_counter() + 2.0
            while len(waits) < 20:
                t0 = time.perf_counter()
                torch.cuda.synchronize()
                waits.append(time.perf_counter() - t0)
                time.sleep(max(0.0, (t_end - time.perf_counter()) / (21 - len(waits))))
        finally:
            stop.set()
            th.join(30)
        assert not th.is_alive()
        print(f"life {life_us} us: {calls[0]} calls; synchronize waits ms: "
              f"max {1e3 * max(waits):.3f} median {1e3 * sorted(waits)[10]:.3f}")
        assert not bad, bad[:5]
        assert calls[0] > 20000                           # the traffic really was steady
        return waits
    try:
        sys.setswitchinterval(5e-5)
        waits = run(1000)
        assert max(waits) <= 2.0e-3, waits                # life (1 ms) + 1 ms
        # control: a 20 ms life and a 50 ms idle timeout; one call, then the
        # synchronisation waits for the live server's remaining life
        assert lib.zp_parse_one_config(ctx, 50000) == 0
        assert lib.zp__one_test_hooks(ctx, 20000, 0, 0) == 0
        rec = np.zeros(1, R.RECORD_DTYPE)
        ext = np.zeros((2, 16), np.uint8)
        assert lib.zp_parse_one(ctx, ctypes.addressof(bufs[0]), len(frames[0]),
                                rec.ctypes.data, ext.ctypes.data) == want[0][0]
        t0 = time.perf_counter()
        torch.cuda.synchronize()
        assert time.perf_counter() - t0 >= 10e-3
    finally:
        sys.setswitchinterval(old_si)
        lib.zp__one_test_hooks(ctx, 1000, 0, 0)          # the device server's default life
        lib.zp_ctx_destroy(ctx)


def test_parse_one_giveup_retires_request(zp):
    """when zp_parse_one gives up waiting (test hook: a 300 us
    give-up, a 30 ms stall queued in front of the server), the request is
    retired and the servers are stopped before the call returns, so a late
    server never answers it from a frame the next call is rewriting; the next
    calls, on other frames, equal the oracle."""
    import time
    R = zp.records
    frames = _c5_frames(zp, 64, seed=9)
    want = [orc.parse_one(f) for f in frames]
    lib = zp._lib.hip()
    ctx = lib.zp_ctx_create(0, 1 << 20)
    assert ctx
    rec = np.zeros(1, R.RECORD_DTYPE)
    ext = np.zeros((2, 16), np.uint8)

    def call(i):
        buf = ctypes.create_string_buffer(frames[i], max(len(frames[i]), 1))
        return lib.zp_parse_one(ctx, ctypes.addressof(buf), len(frames[i]),
                                rec.ctypes.data, ext.ctypes.data)
    try:
        for rep in range(3):
            assert lib.zp__one_test_hooks(ctx, 0, 300, 30000) == 0
            t0 = time.perf_counter()
            assert call(rep) == -2                        # gave up
            dt = time.perf_counter() - t0
            assert dt >= 0.025, dt                        # ... after the stall drained
            assert b"no answer" in lib.zp_last_error()
            assert lib.zp__one_test_hooks(ctx, 0, 10_000_000, 0) == 0
            for i in range(8, 64):
                err, wrec, wext = want[i]
                assert call(i) == err and rec.tobytes() == orc.pack(wrec, wext).tobytes(), (rep, i)
                assert ext.tobytes() == wext.view(np.uint8).tobytes(), (rep, i)
    finally:
        lib.zp__one_test_hooks(ctx, 0, 0, 0)              # no stall
        lib.zp_ctx_destroy(ctx)


def test_parse_one_life_rotation(zp):
    """A 200 us server life: under back-to-back calls the host queues a new
    generation of the device's server behind the old one every ~100 us of its
    clock and retires the old one, each wave starting from its slot's
    acknowledgement word; 6,000 answers equal the oracle's (none lost, none
    answered twice from a rewritten frame), and the rotations happened."""
    R = zp.records
    frames = _c5_frames(zp, 512, seed=13)
    want = [orc.parse_one(f) for f in frames]
    lib = zp._lib.hip()
    ctx = lib.zp_ctx_create(0, 1 << 20)
    assert ctx
    rec = np.zeros(1, R.RECORD_DTYPE)
    ext = np.zeros((2, 16), np.uint8)
    rng = np.random.default_rng(4)
    st0, st1 = np.zeros(3, np.uint64), np.zeros(3, np.uint64)
    try:
        assert lib.zp__one_test_hooks(ctx, 200, 0, 0) == 0
        lib.zp__one_stats(ctx, st0.ctypes.data)
        for k, i in enumerate(rng.integers(0, len(frames), 6000)):
            f = frames[i]
            buf = ctypes.create_string_buffer(f, max(len(f), 1))
            rc = lib.zp_parse_one(ctx, ctypes.addressof(buf), len(f), rec.ctypes.data,
                                  ext.ctypes.data)
            err, wrec, wext = want[i]
            assert rc == err and rec.tobytes() == orc.pack(wrec, wext).tobytes(), (k, int(i), rc)
            assert ext.tobytes() == wext.view(np.uint8).tobytes(), (k, int(i))
        lib.zp__one_stats(ctx, st1.ctypes.data)
        assert st1[1] - st0[1] >= 20, (st0, st1)         # rotations
    finally:
        lib.zp__one_test_hooks(ctx, 1000, 0, 0)          # the device server's default life
        lib.zp_ctx_destroy(ctx)


def test_parser_threads_and_current_device(zp, golden):
    """PacketParser.parse from 8 threads at once: each call leases a context
    of the current device's pool (no global lock), results equal the
    single-thread ones; the pool belongs to torch's current device."""
    import threading
    P = zp.parser
    frames = [bytes.fromhex(fx["bytes"]) for fx in golden["fixtures"]]
    frames += _c5_frames(zp, 200, seed=21)

    def result(f):
        try:
            return P.PacketParser.parse(f).debug()
        except P.ZeroPacketError as e:
            return repr(e)
    want = [result(f) for f in frames]
    assert zp._lib.hip().zp_device_current() == torch.cuda.current_device()
    got, errs = {}, []

    def worker(t):
        try:
            got[t] = [result(f) for f in frames[t::3] + frames]
        except Exception as e:                            # surfaced below
            errs.append(repr(e))
    ths = [threading.Thread(target=worker, args=(t,)) for t in range(8)]
    for t in ths:
        t.start()
    for t in ths:
        t.join(120)
    assert not errs, errs
    for t in range(8):
        assert got[t] == want[t::3] + want, t
    pool = P._POOLS[torch.cuda.current_device()]
    assert pool.device == torch.cuda.current_device()
    assert 1 <= len(pool.all) <= 8 and all(pool.all)
    P.quiesce()


def test_parse_one_contexts_share_the_device_server(zp):
    """12 contexts on 12 threads call zp_parse_one at once: they share the
    device's one server kernel (one wave per context slot), so none waits
    behind another's resident kernel on a hardware queue (with a kernel per
    context, the ones past the process' 4 hardware queues waited up to a
    whole life); contexts created and destroyed while the others run are
    served too. Every answer equals the oracle's. (The per-call times of
    12 Python threads are GIL-bound, so they are printed, not asserted; the
    thread scaling is measured in C++ by tools/parse_one_latency.py.)"""
    import sys
    import threading
    import time
    R = zp.records
    frames = _c5_frames(zp, 256, seed=31)
    want = [orc.parse_one(f) for f in frames]
    packed = [orc.pack(w[1], w[2]).tobytes() for w in want]
    bufs = [ctypes.create_string_buffer(f, len(f)) for f in frames]
    lib = zp._lib.hip()
    bad, dts = [], [[] for _ in range(12)]
    go = threading.Barrier(12)

    def worker(t):
        rec = np.zeros(1, R.RECORD_DTYPE)
        ext = np.zeros((2, 16), np.uint8)
        for life in range(2 if t % 4 == 0 else 1):       # some contexts come and go
            ctx = lib.zp_ctx_create(0, 1 << 20)
            try:
                if life == 0:
                    go.wait()
                for k in range(1500):
                    i = (k * 7 + t) % len(frames)
                    t0 = time.perf_counter()
                    rc = lib.zp_parse_one(ctx, ctypes.addressof(bufs[i]), len(frames[i]),
                                          rec.ctypes.data, ext.ctypes.data)
                    dts[t].append(time.perf_counter() - t0)
                    if rc != want[i][0] or rec.tobytes() != packed[i]:
                        bad.append((t, k, i, rc))
            finally:
                lib.zp_ctx_destroy(ctx)
    old_si = sys.getswitchinterval()
    sys.setswitchinterval(5e-5)
    try:
        ths = [threading.Thread(target=worker, args=(t,)) for t in range(12)]
        for th in ths:
            th.start()
        for th in ths:
            th.join(120)
    finally:
        sys.setswitchinterval(old_si)
    assert not bad, bad[:5]
    allv = np.sort(np.concatenate([np.array(v) for v in dts]))
    p50, p99 = allv[len(allv) // 2], allv[int(len(allv) * 0.99)]
    print(f"{len(allv)} calls: p50 {1e6 * p50:.1f} us, p99 {1e6 * p99:.1f} us, "
          f"max {1e3 * allv[-1]:.3f} ms")
    assert len(allv) == 12 * 1500 + 3 * 1500


def test_parse_one_more_contexts_than_server_slots(zp):
    """70 live contexts on one device: the first 64 get a slot of the device's
    server, the rest fall back to one batch launch per call; every context's
    answers equal the oracle's, and destroying contexts frees their slots
    for new ones."""
    R = zp.records
    frames = _c5_frames(zp, 140, seed=41)
    want = [orc.parse_one(f) for f in frames]
    lib = zp._lib.hip()
    rec = np.zeros(1, R.RECORD_DTYPE)
    ext = np.zeros((2, 16), np.uint8)
    ctxs = []

    def call(ctx, i):
        buf = ctypes.create_string_buffer(frames[i], len(frames[i]))
        rc = lib.zp_parse_one(ctx, ctypes.addressof(buf), len(frames[i]), rec.ctypes.data,
                              ext.ctypes.data)
        err, wrec, wext = want[i]
        assert rc == err and rec.tobytes() == orc.pack(wrec, wext).tobytes(), (i, rc, err)
        assert ext.tobytes() == wext.view(np.uint8).tobytes(), i
    try:
        for k in range(70):
            ctxs.append(lib.zp_ctx_create(0, 1 << 16))
            assert ctxs[-1]
            call(ctxs[-1], k)
        for k, c in enumerate(ctxs):                       # all of them again, interleaved
            call(c, 70 + k)
        for c in ctxs[:10]:
            lib.zp_ctx_destroy(c)
        ctxs = ctxs[10:]
        for k in range(10):                                # new contexts take the freed slots
            ctxs.append(lib.zp_ctx_create(0, 1 << 16))
            call(ctxs[-1], 130 + k)
    finally:
        for c in ctxs:
            lib.zp_ctx_destroy(c)


def test_probe_tiles_stays_in_bounds(zp):
    """zp_probe_tiles_device (bench.py's placement probe) on a batch whose
    frame count is not a multiple of 64: the record stores stop at n (a
    guard after the records is untouched) and the read-only form writes
    nothing there."""
    d = dev()
    n = 1000
    a, o, l_ = zp.batch.generate("c3", n, device=d)
    buf = torch.full((n + 64, 8), 0xA5, dtype=torch.uint8, device=d)
    sink = torch.zeros(1, dtype=torch.int32, device=d)
    lib = zp._lib.hip()
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    nb = a.numel() // 16 * 16
    assert lib.zp_probe_tiles_device(a.data_ptr(), nb, n, o.data_ptr(), l_.data_ptr(), None,
                                     sink.data_ptr(), s) == 0
    torch.cuda.synchronize()
    assert (buf == 0xA5).all()
    assert lib.zp_probe_tiles_device(a.data_ptr(), nb, n, o.data_ptr(), l_.data_ptr(),
                                     buf.data_ptr(), sink.data_ptr(), s) == 0
    torch.cuda.synchronize()
    assert (buf[n:] == 0xA5).all() and not (buf[:n] == 0xA5).all(1).all()
