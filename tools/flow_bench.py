"""Times the flow table (zp_flow_aggregate_device) beside the composition a
caller writes without it, in one process.

    python tools/flow_bench.py [--configs c3,c4] [--packets 16777216] [--reps 5] [--runs 5]
                               [--extremes 1] [--yardstick 1] [--log profiles/flow_bench.log]

Rows per config (HIP events; each run is the median of --reps repetitions
after warm-up, a row reports the median of --runs runs and their min-max
spread), 5-tuple key:
  flows        flows.aggregate(check=False) into preallocated outputs, with F
  extract      columns.extract of the six key columns: the floor for the key pass
  composed     the same extract, the rows glued to 40 bytes (five int64 words),
               torch.unique(dim=0, return_inverse, return_counts) and scatter_add
               of the bytes; its sorted counts must equal the sorted `packets`
Extremes (--extremes 1): one flow (every descriptor points at one frame:
maximum contention) with and without the in-wave combining; 65,536 flows of
256 frames each (the first 65,536 c2 frames over and over); and c2, whose
frames the generator makes pairwise distinct, as it does those of c3 and c4
(F = n: maximum table traffic).
"""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KEY_COLS = ["src_addr", "dest_addr", "src_port", "dest_port", "l4_proto", "ip_version"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c3,c4")
    ap.add_argument("--packets", type=int, default=1 << 24)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--extremes", type=int, default=1)
    ap.add_argument("--yardstick", type=int, default=1)
    ap.add_argument("--log", default="")
    a = ap.parse_args()
    zp = importlib.import_module("zero-packet_amd")
    lib = zp._lib.hip()
    d = torch.device("cuda:0")
    n = a.packets
    s = torch.cuda.current_stream(d)
    lines = [f"flow_bench: {n} frames, {torch.cuda.get_device_name(d)}, 5-tuple key, per row the "
             f"median of {a.runs} runs (each the median of {a.reps} repetitions) and the runs' min-max"]

    def say(x):
        print(x, flush=True)
        lines.append(x)

    def timed(fn, reps=None, runs=None):
        out = []
        for _ in range(runs or a.runs):
            fn()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                  for _ in range(reps or a.reps)]
            for x, y in ev:
                x.record(s)
                fn()
                y.record(s)
            torch.cuda.synchronize()
            out.append(float(np.median([x.elapsed_time(y) for x, y in ev])))
        return float(np.median(out)), min(out), max(out)

    def fmt(t):
        return f"{t[0]:9.3f} ms [{t[1]:8.3f} - {t[2]:8.3f}]"

    def outputs(m):
        return {"count": torch.zeros(4, dtype=torch.int64, device=d),
                "flows": torch.empty((m, 64), dtype=torch.uint8, device=d),
                "flow_of": torch.empty(n, dtype=torch.int32, device=d),
                "scratch": torch.empty(int(lib.zp_flow_scratch_bytes(n, m)), dtype=torch.uint8,
                                       device=d)}

    def flows_row(name, arena, offs, lens, recs, reps=None, runs=None):
        out = outputs(n)
        t = timed(lambda: zp.flows.aggregate(arena, offs, lens, recs, out=out, check=False), reps, runs)
        cnt = [int(v) for v in out["count"].tolist()]
        say(f"{name:<12s} flows {fmt(t)}   {n / t[0] / 1e6:7.2f} Gframes/s   F {cnt[0]}   keyed "
            f"{cnt[1]}   overflow {cnt[3]}")
        return t, out, cnt

    for cfg in [c for c in a.configs.split(",") if c]:          # --configs "": the extremes only
        arena, offs, lens = zp.batch.generate(cfg, n, device=d)
        recs, _ = zp.batch.parse_batch(arena, offs, lens)
        torch.cuda.synchronize()
        say(f"--- {cfg}: {arena.numel() / 1e9:.2f} GB arena, {arena.numel() / n:.0f} B per frame")
        t_fl, out, cnt = flows_row(cfg, arena, offs, lens, recs)
        head = zp.columns.extract(arena[:1 << 20], offs[:256], lens[:256], recs[:256], names=KEY_COLS,
                                  check=False)
        cols = {k: torch.empty((n,) + tuple(v.shape[1:]), dtype=v.dtype, device=d)
                for k, v in head.items()}
        t_ext = timed(lambda: zp.columns.extract(arena, offs, lens, recs, names=KEY_COLS, out=cols,
                                                 check=False))
        say(f"{cfg:<12s} extract of the six key columns {fmt(t_ext)}   flows/extract "
            f"{t_fl[0] / t_ext[0]:5.2f}")
        if a.yardstick:
            rows = torch.zeros((n, 40), dtype=torch.uint8, device=d)
            nbytes = lens.to(torch.int64)

            def composed():
                c = zp.columns.extract(arena, offs, lens, recs, names=KEY_COLS, out=cols, check=False)
                rows[:, 0:16] = c["src_addr"]
                rows[:, 16:32] = c["dest_addr"]
                rows[:, 32:34] = c["src_port"].view(torch.uint8).view(n, 2)
                rows[:, 34:36] = c["dest_port"].view(torch.uint8).view(n, 2)
                rows[:, 36] = c["l4_proto"]
                rows[:, 37] = c["ip_version"]
                keys, inv, counts = torch.unique(rows.view(torch.int64), dim=0, return_inverse=True,
                                                 return_counts=True)
                total = torch.zeros(keys.shape[0], dtype=torch.int64, device=d)
                total.scatter_add_(0, inv.flatten(), nbytes)
                return counts, total
            x, y = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            composed()
            x.record(s)
            counts, total = composed()
            y.record(s)
            torch.cuda.synchronize()
            once = x.elapsed_time(y)
            # every frame of the generated configs is keyed: the composition sees the same flows
            ent = zp.flows.to_numpy(zp.flows.FlowTable(out["count"], out["flows"], None))
            same = cnt[1] == n and np.array_equal(np.sort(counts.cpu().numpy()),
                                                  np.sort(ent["packets"].astype(np.int64))) and \
                np.array_equal(np.sort(total.cpu().numpy()), np.sort(ent["bytes"].astype(np.int64)))
            del counts, total
            few = once > 2000.0                          # a slow yardstick is timed once per run
            t_cmp = timed(composed, reps=1 if few else a.reps, runs=2 if few else a.runs)
            say(f"{cfg:<12s} extract + glue + torch.unique(dim=0) + scatter_add {fmt(t_cmp)}"
                f"{' (2 runs of 1)' if few else ''}   composed/flows {t_cmp[0] / t_fl[0]:6.2f}   "
                f"faster outside the spread: {'yes' if t_fl[2] < t_cmp[1] else 'no'}   same counts "
                f"and bytes: {same}")
            del rows, nbytes
        del arena, offs, lens, recs, out, cols
        torch.cuda.empty_cache()
    if a.extremes:
        arena, offs, lens = zp.batch.generate("c5", 64, device=d)
        recs, _ = zp.batch.parse_batch(arena, offs, lens)
        k = int((zp.batch.record_flags(recs) & (zp.records.F_IPV4 | zp.records.F_IPV6)).nonzero()[0])
        offs1, lens1 = offs[k].repeat(n), lens[k].repeat(n)
        recs1 = recs[k:k + 1].repeat(n, 1)
        say("--- one flow: every descriptor points at one frame")
        for on in (1, 0):
            was = lib.zp__flow_combine(on)
            try:
                # without the combining one call takes about a second: two runs of one
                flows_row("combine on" if on else "combine off (2 runs of 1)", arena, offs1, lens1,
                          recs1, *(() if on else (1, 2)))
            finally:
                lib.zp__flow_combine(was)
        del arena, offs, lens, recs, offs1, lens1, recs1
        torch.cuda.empty_cache()
        arena, offs, lens = zp.batch.generate("c2", n, device=d)
        recs, _ = zp.batch.parse_batch(arena, offs, lens)
        torch.cuda.synchronize()
        m = 1 << 16
        say(f"--- c2, the first {m} frames over and over: {m} flows of {n // m} frames, "
            f"neighbouring lanes on different flows")
        pick = torch.arange(n, device=d) % m
        flows_row("combine on", arena, offs[pick], lens[pick], recs[pick])
        del pick
        say("--- c2: 64-B frames, the generator's flows")
        for on in (1, 0):
            was = lib.zp__flow_combine(on)
            try:
                flows_row("combine on" if on else "combine off", arena, offs, lens, recs)
            finally:
                lib.zp__flow_combine(was)
    if a.log:
        with open(a.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
