"""Times the route stage (zp_route_device) beside what it is set against, on
the same frames in one process.

    python tools/route_bench.py [--configs c3,c4] [--packets 16777216]
                                [--prefixes 1,1024,65536,1048576] [--reps 5] [--runs 5]
                                [--log profiles/route_bench.log]

Tables (fixed seed), P prefixes each, in two shapes:
  deep     prefixes drawn from the batch's own destination addresses, half at
           /24 and half at /32 (c3, IPv4) or /48 and /64 (c4, IPv6): the frames
           they were drawn from walk to the bottom of the trie;
  shallow  random /16 to /24 prefixes: most frames stop at the root or one
           level down.
Each row states the loads per frame its table costs (the walk of zp_route.h
replayed in numpy over a sample of the batch) and the share of frames matched.
Rows per config (HIP events; each run is the median of --reps repetitions
after warm-up, a row reports the median of --runs runs and their min-max):
  route      RouteTable.run(check=False): value_of and mask in one launch
  extract    columns.extract of ip_version and dest_addr
  classify   a RuleTable of one one-term rule on dest_addr writing rule_of and
             mask: it stages the same header and writes the same outputs, so
             route / classify at P = 1 is the cost of the walk
  searchsorted (c3 only) what a caller writes without the stage: extract
             dest_addr, the addresses as big-endian integers, one
             torch.searchsorted pass per distinct prefix length in ascending
             order, the longest hit kept. Its answers must equal route's.
             Nothing comparable exists for IPv6 (a 128-bit key has no torch
             integer type): the c4 rows say so.
"""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HDR, ROOT_ENTRIES = 16, 65536          # zp_route.h: RT_HDR, RT_ROOT (dwords)


def truncate(addr, lens):
    """addr uint8 [P, 16] with everything past lens[k] bits cleared."""
    bit = np.arange(128)[None, :] < lens[:, None]
    return addr & np.packbits(bit, axis=1)


def make_prefixes(zp, shape, version, count, sample, rng):
    """PREFIX_DTYPE [<= count]: distinct prefixes of one shape; sample: uint8
    [count, 16] addresses of the batch."""
    if shape == "deep":
        pair = (24, 32) if version == 4 else (48, 64)
        lens = np.where(np.arange(count) % 2 == 0, pair[0], pair[1])
        addr = sample[:count].copy()
    else:
        lens = rng.integers(16, 25, count)
        addr = rng.integers(0, 256, (count, 16)).astype(np.uint8)
    if version == 4:
        addr[:, 4:] = 0
    addr = truncate(addr, lens)
    key = np.concatenate([lens[:, None].astype(np.uint8), addr], axis=1)
    _, first = np.unique(key, axis=0, return_index=True)
    first.sort()
    enc = np.zeros(len(first), zp.routes.PREFIX_DTYPE)
    enc["addr"], enc["len"], enc["version"] = addr[first], lens[first], version
    enc["value"] = np.arange(len(first))
    return enc


def replay(table, addr, version):
    """(value uint32 [m], loads int [m]): the walk of zp_route.h over the
    host table for addresses uint8 [m, 16]."""
    T = table.view("<u4")
    m = len(addr)
    e = T[HDR + (ROOT_ENTRIES if version == 6 else 0) + (addr[:, 0].astype(np.int64) << 8) + addr[:, 1]]
    loads = np.ones(m, np.int64)
    for k in range(2, 4 if version == 4 else 16):
        go = (e & 0x80000000) != 0
        if not go.any():
            break
        node = (e[go] & 0x7FFFFFFF).astype(np.int64)
        e[go] = T[HDR + 2 * ROOT_ENTRIES + node * 256 + addr[go, k]]
        loads[go] += 1
    return np.where(e == 0x7FFFFFFF, 0xFFFFFFFF, e).astype(np.uint32), loads


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c3,c4")
    ap.add_argument("--packets", type=int, default=1 << 24)
    ap.add_argument("--prefixes", default="1,1024,65536,1048576")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--log", default="")
    a = ap.parse_args()
    zp = importlib.import_module("zero-packet_amd")
    d = torch.device("cuda:0")
    n = a.packets
    s = torch.cuda.current_stream(d)
    counts = [int(x) for x in a.prefixes.split(",")]
    lines = []

    def say(x):
        print(x, flush=True)
        lines.append(x)
    say(f"route_bench: {n} frames, {torch.cuda.get_device_name(d)}, per row the median of {a.runs} "
        f"runs (each the median of {a.reps} repetitions) and the runs' min-max")

    def timed(fn):
        out = []
        for _ in range(a.runs):
            fn()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                  for _ in range(a.reps)]
            for x, y in ev:
                x.record(s)
                fn()
                y.record(s)
            torch.cuda.synchronize()
            out.append(float(np.median([x.elapsed_time(y) for x, y in ev])))
        return float(np.median(out)), min(out), max(out)

    def fmt(t):
        return f"{t[0]:8.3f} ms [{t[1]:8.3f} - {t[2]:8.3f}]"

    def ratio(x, y):
        """x / y of two timed() results with the range the runs' extremes give."""
        return f"{x[0] / y[0]:5.2f} [{x[1] / y[2]:5.2f} - {x[2] / y[1]:5.2f}]"

    words = (n + 63) // 64
    for cfg in [c for c in a.configs.split(",") if c]:
        version = 6 if cfg == "c4" else 4
        rng = np.random.default_rng(20250321)
        arena, offs, lens = zp.batch.generate(cfg, n, device=d)
        recs, _ = zp.batch.parse_batch(arena, offs, lens)
        torch.cuda.synchronize()
        say(f"--- {cfg}: IPv{version}, {arena.numel() / 1e9:.2f} GB arena, {arena.numel() / n:.0f} B per frame")
        out = {"value_of": torch.empty(n, dtype=torch.int32, device=d),
               "mask": torch.empty(words, dtype=torch.int64, device=d),
               "status": torch.zeros(1, dtype=torch.int64, device=d)}
        cols_out = {"ip_version": torch.empty(n, dtype=torch.uint8, device=d),
                    "dest_addr": torch.empty((n, 16), dtype=torch.uint8, device=d)}

        def extract():
            return zp.columns.extract(arena, offs, lens, recs, names=["ip_version", "dest_addr"],
                                      out=cols_out, check=False)
        t_ext = timed(extract)
        say(f"{cfg} extract of ip_version and dest_addr {fmt(t_ext)}")
        dest = cols_out["dest_addr"]
        pick = torch.from_numpy(rng.choice(n, max(counts), replace=False)).to(d)
        sample = dest[pick].cpu().numpy()                # the deep tables' addresses
        probe_at = torch.from_numpy(rng.choice(n, min(n, 1 << 16), replace=False)).to(d)
        probe = dest[probe_at].cpu().numpy()
        # (b) one one-term rule on the same column
        S = zp.select.Select
        net = "128.0.0.0/1" if version == 4 else "8000::/1"
        rules = zp.classify.RuleTable([S().where("dest_addr", prefix=net)], d)
        cls_out = {"rule_of": torch.empty(n, dtype=torch.int32, device=d), "mask": out["mask"],
                   "status": torch.zeros(1, dtype=torch.int64, device=d)}
        t_cls = timed(lambda: rules.run(arena, offs, lens, recs, want=("rule_of", "mask"), out=cls_out,
                                        check=False))
        say(f"{cfg} classify, one rule `dest_addr in {net}`, rule_of and mask {fmt(t_cls)}")
        del cls_out
        for shape in ("deep", "shallow"):
            for P in counts:
                enc = make_prefixes(zp, shape, version, P, sample, rng)
                table = zp.routes.RouteTable(enc, d)
                value, loads = replay(table.table_host, probe, version)
                best = timed(lambda: table.run(arena, offs, lens, recs, out=out, check=False))
                table.run(arena, offs, lens, recs, out=out, check=False)
                torch.cuda.synchronize()
                assert int(out["status"][0]) == 0
                got = out["value_of"].clone()
                matched = float((got != -1).sum()) / n
                say(f"{cfg} {shape:7s} P={len(enc):<8d} table {table.table_host.size / 2**20:8.1f} MiB   "
                    f"loads/frame {loads.mean():5.2f}   matched {100 * matched:5.1f} %   route "
                    f"{fmt(best)}   {n / best[0] / 1e6:5.2f} Gframes/s   "
                    f"route/extract {ratio(best, t_ext)}   route/classify {ratio(best, t_cls)}")
                # the replayed walk's answers on the probe frames are the kernel's
                assert np.array_equal(value, got[probe_at].cpu().numpy().view(np.uint32))
                if version == 4:
                    # (c) one searchsorted pass per distinct length, the longest hit kept
                    by_len = []
                    for L in sorted(set(enc["len"].tolist())):
                        p = enc[enc["len"] == L]
                        key = (p["addr"][:, :4].astype(np.int64) * [1 << 24, 1 << 16, 1 << 8, 1]).sum(1) >> (32 - L)
                        order = np.argsort(key)
                        by_len.append((L, torch.from_numpy(key[order]).to(d),
                                       torch.from_numpy(p["value"][order].astype(np.int32)).to(d)))
                    base = torch.empty(n, dtype=torch.int32, device=d)

                    def searchsorted():
                        a4 = extract()["dest_addr"][:, :4].to(torch.int64)
                        addr = (a4[:, 0] << 24) | (a4[:, 1] << 16) | (a4[:, 2] << 8) | a4[:, 3]
                        base.fill_(-1)
                        for L, keys, vals in by_len:
                            k = addr >> (32 - L)
                            pos = torch.searchsorted(keys, k).clamp_(max=keys.numel() - 1)
                            base.copy_(torch.where(keys[pos] == k, vals[pos], base))
                    t_ss = timed(searchsorted)
                    same = torch.equal(base, got)
                    say(f"{cfg} {shape:7s} P={len(enc):<8d} searchsorted, {len(by_len)} lengths {fmt(t_ss)}   "
                        f"searchsorted/route {ratio(t_ss, best)}   route faster outside the spread: "
                        f"{'yes' if best[2] < t_ss[1] else 'no'}   same answers: {same}")
                    del by_len, base
                else:
                    say(f"{cfg} {shape:7s} P={len(enc):<8d} searchsorted: nothing comparable for IPv6 "
                        f"(no 128-bit integer keys in torch)")
                del table, got
                torch.cuda.empty_cache()
        del arena, offs, lens, recs, out, cols_out, dest
        torch.cuda.empty_cache()
    if a.log:
        with open(a.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
