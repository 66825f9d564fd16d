"""Times the persistent flow table (flows.Table) beside zp_flow_aggregate_device
on the same frames, in one process.

    python tools/flow_table_bench.py [--configs c3,c4] [--packets 16777216] [--reps 5] [--runs 5]
                                     [--rows abcdef] [--log profiles/flow_table_bench.log]

HIP events; each run is the median of --reps repetitions after a warm-up, a
row reports the median of --runs runs and their min-max. The 5-tuple key.
  (a) the first update of an empty table (the init is outside the timed span)
  (b) a second update of the same batch: every frame belongs to a known flow
  (c) 65,536 flows of 256 frames (the first 65,536 c2 frames over and over)
  (d) one flow (every descriptor points at one frame)
  (e) a retire of every other flow of the table (a), and a retire of none
      (the table is restored from a copy outside the timed span)
  (f) 16 updates of packets / 16 frames each, against what a caller does
      without the table: aggregate per batch, torch.unique(dim=0) over the
      old and new 40-byte keys, scatter_add of the counters and the flow_of
      re-map
The yardstick of every row is flows.aggregate on the same frames.
"""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c3,c4")
    ap.add_argument("--packets", type=int, default=1 << 24)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--rows", default="abcdef")
    ap.add_argument("--log", default="")
    a = ap.parse_args()
    zp = importlib.import_module("zero-packet_amd")
    lib = zp._lib.hip()
    d = torch.device("cuda:0")
    n = a.packets
    s = torch.cuda.current_stream(d)
    lines = [f"flow_table_bench: {n} frames, {torch.cuda.get_device_name(d)}, 5-tuple key, per row the "
             f"median of {a.runs} runs (each the median of {a.reps} repetitions) and the runs' min-max"]

    def say(x):
        print(x, flush=True)
        lines.append(x)

    def timed(fn, before=None, reps=None, runs=None):
        out = []
        for _ in range(runs or a.runs):
            if before:
                before()
            fn()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                  for _ in range(reps or a.reps)]
            for x, y in ev:
                if before:
                    before()
                x.record(s)
                fn()
                y.record(s)
            torch.cuda.synchronize()
            out.append(float(np.median([x.elapsed_time(y) for x, y in ev])))
        return float(np.median(out)), min(out), max(out)

    def fmt(t):
        return f"{t[0]:9.3f} ms [{t[1]:8.3f} - {t[2]:8.3f}]"

    def versus(t, y):
        return f"{t[0] / y[0]:5.2f} x aggregate, " + \
            ("faster" if t[2] < y[1] else "slower" if t[1] > y[2] else "within the spread")

    def agg_out(m, cap):
        return {"count": torch.zeros(4, dtype=torch.int64, device=d),
                "flows": torch.empty((cap, 64), dtype=torch.uint8, device=d),
                "flow_of": torch.empty(m, dtype=torch.int32, device=d),
                "scratch": torch.empty(int(lib.zp_flow_scratch_bytes(m, cap)), dtype=torch.uint8, device=d)}

    def upd_out(m):
        return {"count": torch.zeros(8, dtype=torch.int64, device=d),
                "flow_of": torch.empty(m, dtype=torch.int32, device=d),
                "scratch": torch.empty(int(lib.zp_flow_update_scratch_bytes(m)), dtype=torch.uint8, device=d)}

    def first_and_second(name, arena, offs, lens, recs, cap, keep=False):
        """Rows (a) and (b) for one batch; returns the table after two updates."""
        out = agg_out(n, cap)
        y = timed(lambda: zp.flows.aggregate(arena, offs, lens, recs, max_flows=cap, out=out, check=False))
        f = int(out["count"][0])
        say(f"{name:<10s} aggregate            {fmt(y)}   F {f}")
        del out
        tab, uo = zp.flows.Table(cap, d), upd_out(n)
        upd = lambda: tab.update(arena, offs, lens, recs, out=uo, check=False)
        if "a" in a.rows:
            t = timed(upd, before=tab.init)
            c = [int(v) for v in uo["count"].tolist()]
            say(f"{name:<10s} (a) first update     {fmt(t)}   {versus(t, y)}   F {c[0]} admitted {c[1]}")
            assert c[0] == f == c[1] and c[7] == 0
        tab.init()
        upd()
        if "b" in a.rows:
            t = timed(upd)
            c = [int(v) for v in uo["count"].tolist()]
            say(f"{name:<10s} (b) second update    {fmt(t)}   {versus(t, y)}   F {c[0]} admitted {c[1]}")
            assert c[0] == f and c[1] == 0 and c[7] == 0
        del uo
        return (tab, y) if keep else None

    for cfg in [c for c in a.configs.split(",") if c]:
        arena, offs, lens = zp.batch.generate(cfg, n, device=d)
        recs, _ = zp.batch.parse_batch(arena, offs, lens)
        torch.cuda.synchronize()
        say(f"--- {cfg}: {arena.numel() / 1e9:.2f} GB arena, {arena.numel() / n:.0f} B per frame")
        tab = None
        if set("abe") & set(a.rows):
            tab, y = first_and_second(cfg, arena, offs, lens, recs, n, keep=True)
        if "e" in a.rows:
            f, _ = tab.header()
            tab.flows.view(torch.int64).view(-1, 8)[1:f:2, 6] |= 1 << 56     # FIN on every other flow
            copy = (tab.table.clone(), tab.flows.clone())
            ro = {"count": torch.zeros(2, dtype=torch.int64, device=d),
                  "retired": torch.empty((n, 64), dtype=torch.uint8, device=d),
                  "remap": torch.empty(n, dtype=torch.int32, device=d),
                  "scratch": torch.empty(int(lib.zp_flow_retire_scratch_bytes(n)), dtype=torch.uint8,
                                         device=d)}

            def restore():
                tab.table.copy_(copy[0])
                tab.flows.copy_(copy[1])
            for what, any_ in (("every other flow", 1), ("no flow", 0)):
                t = timed(lambda: tab.retire(None, any_, out=ro), before=restore)
                c = [int(v) for v in ro["count"].tolist()]
                say(f"{cfg:<10s} (e) retire of {what:<17s}{fmt(t)}   {versus(t, y)}   F' {c[0]} retired {c[1]}")
            del copy, ro
        del tab
        torch.cuda.empty_cache()
        if "f" in a.rows:
            k = 16
            m = n // k
            out = agg_out(n, n)
            y = timed(lambda: zp.flows.aggregate(arena, offs, lens, recs, out=out, check=False))
            want = np.sort(zp.flows.to_numpy(zp.flows.FlowTable(out["count"], out["flows"], None))
                           ["packets"].astype(np.int64))
            del out
            tab, uo = zp.flows.Table(n, d), upd_out(m)

            def updates():
                for j in range(k):
                    q = slice(j * m, (j + 1) * m)
                    tab.update(arena, offs[q], lens[q], recs[q], out=uo, check=False)
            t = timed(updates, before=tab.init)
            got = np.sort(zp.flows.state_packets(tab.to_numpy()).astype(np.int64))
            say(f"{cfg:<10s} (f) {k} updates of {m}  {fmt(t)}   {versus(t, y)}   same packets as "
                f"aggregate over all: {np.array_equal(got, want)}")
            del tab, uo
            mo = agg_out(m, m)

            def merged():
                tk = torch.empty((0, 5), dtype=torch.int64, device=d)
                tp = tb = torch.empty(0, dtype=torch.int64, device=d)
                for j in range(k):
                    q = slice(j * m, (j + 1) * m)
                    r = zp.flows.aggregate(arena, offs[q], lens[q], recs[q], out=mo, check=False)
                    f = int(r.count[0])                     # the caller has to know F: a read-back
                    ent = r.flows[:f]
                    keys = ent[:, :40].contiguous().view(torch.int64)
                    pk = ent[:, 48:52].contiguous().view(torch.int32).flatten().to(torch.int64)
                    by = ent[:, 56:64].contiguous().view(torch.int64).flatten()
                    uk, inv = torch.unique(torch.cat([tk, keys]), dim=0, return_inverse=True)
                    np_ = torch.zeros(uk.shape[0], dtype=torch.int64, device=d)
                    nb = torch.zeros(uk.shape[0], dtype=torch.int64, device=d)
                    np_.scatter_add_(0, inv, torch.cat([tp, pk]))
                    nb.scatter_add_(0, inv, torch.cat([tb, by]))
                    flow_of = inv[tk.shape[0]:][r.flow_of.long()]     # every generated frame is keyed
                    tk, tp, tb = uk, np_, nb
                return tp, flow_of
            x, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            merged()
            x.record(s)
            tp, _ = merged()
            z.record(s)
            torch.cuda.synchronize()
            once = x.elapsed_time(z)
            same = np.array_equal(np.sort(tp.cpu().numpy()), want)
            del tp
            few = once > 2000.0
            c = timed(merged, reps=1 if few else a.reps, runs=2 if few else a.runs)
            say(f"{cfg:<10s} (f) aggregate + unique + scatter_add + re-map per batch {fmt(c)}"
                f"{' (2 runs of 1)' if few else ''}   composed/table {c[0] / t[0]:6.2f}   table faster "
                f"outside the spread: {'yes' if t[2] < c[1] else 'no'}   same packets: {same}")
            del mo
        del arena, offs, lens, recs
        torch.cuda.empty_cache()
    if "d" in a.rows:
        arena, offs, lens = zp.batch.generate("c5", 64, device=d)
        recs, _ = zp.batch.parse_batch(arena, offs, lens)
        k = int((zp.batch.record_flags(recs) & (zp.records.F_IPV4 | zp.records.F_IPV6)).nonzero()[0])
        say("--- (d) one flow: every descriptor points at one frame")
        first_and_second("one flow", arena, offs[k].repeat(n), lens[k].repeat(n), recs[k:k + 1].repeat(n, 1), 64)
        del arena, offs, lens, recs
        torch.cuda.empty_cache()
    if "c" in a.rows:
        arena, offs, lens = zp.batch.generate("c2", n, device=d)
        recs, _ = zp.batch.parse_batch(arena, offs, lens)
        torch.cuda.synchronize()
        m = 1 << 16
        say(f"--- (c) c2, the first {m} frames over and over: {m} flows of {n // m} frames")
        pick = torch.arange(n, device=d) % m
        first_and_second("64k flows", arena, offs[pick], lens[pick], recs[pick], m)
    if a.log:
        with open(a.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
