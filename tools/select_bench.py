"""Times select and gather (zp_select_device, zp_gather_frames_device) beside
what a caller has to do without them, in one process.

    python tools/select_bench.py [--configs c3,c4] [--gather-configs c3,c4,c2]
                                 [--packets 16777216] [--reps 10] [--runs 5]
                                 [--log profiles/select_bench.log]

Rows per config (HIP events; each run is the median of --reps repetitions
after warm-up, a row reports the median of --runs runs and their min-max
spread):
  record-only   Select(ok, has tcp|udp) -> idx   beside zp_stats_device over the same records
  5-tuple       src /8 + dest-port range + l4_proto + ip_version -> idx
                beside columns.extract of the four columns + the torch mask ops + nonzero
  gather        packed gather at about 1 %, 50 % and 100 % selectivity (a range on
                l4_checksum picks the share) beside torch.index_select of the three
                descriptor tensors + a device clone of the same byte count
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
    ap.add_argument("--gather-configs", default="c3,c4,c2")
    ap.add_argument("--packets", type=int, default=1 << 24)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--log", default="")
    a = ap.parse_args()
    zp = importlib.import_module("zero-packet_amd")
    S, C = zp.select.Select, zp.columns
    d = torch.device("cuda:0")
    n = a.packets
    s = torch.cuda.current_stream(d)
    lines = [f"select_bench: {n} frames, {torch.cuda.get_device_name(d)}, per row the median of "
             f"{a.runs} runs (each the median of {a.reps} repetitions) and the runs' min-max"]

    def say(x):
        print(x, flush=True)
        lines.append(x)

    def timed(fn):
        runs = []
        for _ in range(a.runs):
            for _ in range(2):
                fn()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                  for _ in range(a.reps)]
            for x, y in ev:
                x.record(s)
                fn()
                y.record(s)
            torch.cuda.synchronize()
            runs.append(float(np.median([x.elapsed_time(y) for x, y in ev])))
        return float(np.median(runs)), min(runs), max(runs)

    def fmt(t):
        return f"{t[0]:8.3f} ms [{t[1]:7.3f} - {t[2]:7.3f}]"

    def outside(x, y):          # faster outside the runs' spread
        return "yes" if x[2] < y[1] else "no"

    configs = a.configs.split(",")
    for cfg in dict.fromkeys(configs + a.gather_configs.split(",")):
        arena, offs, lens = zp.batch.generate(cfg, n, device=d)
        recs, _ = zp.batch.parse_batch(arena, offs, lens)
        torch.cuda.synchronize()
        say(f"--- {cfg}: {arena.numel() / 1e9:.2f} GB arena, {arena.numel() / n:.0f} B per frame")
        out = {"idx": torch.empty(n, dtype=torch.int32, device=d),
               "packed_offs": torch.empty(n, dtype=torch.int64, device=d),
               "count": torch.zeros(2, dtype=torch.int64, device=d),
               "scratch": torch.empty(int(zp._lib.hip().zp_select_scratch_bytes(n)),
                                      dtype=torch.uint8, device=d)}
        if cfg in configs:
            # record-only
            sel = S(ok=True, any_of=("tcp", "udp"))
            counts = torch.zeros(64, dtype=torch.int64, device=d)
            t_sel = timed(lambda: zp.select.run(None, None, lens, recs, sel, want=("idx",), out=out,
                                                check=False))
            t_nolen = timed(lambda: zp.select.run(None, None, None, recs, sel, want=("idx",),
                                                  out=out, check=False))
            t_stats = timed(lambda: zp._lib.hip().zp_stats_device(recs.data_ptr(), n,
                                                                  counts.data_ptr(), s.cuda_stream))
            c = int(out["count"][0])
            say(f"record-only  select {fmt(t_sel)}   without lens {fmt(t_nolen)}   "
                f"zp_stats_device {fmt(t_stats)}   select/stats {t_sel[0] / t_stats[0]:5.2f}   "
                f"selected {c / n:6.1%}")
            # 5-tuple: the first accepted IP frame's /8, a port range, its l4_proto
            names = ["src_addr", "dest_port", "l4_proto", "ip_version"]
            head = C.extract(arena[:1 << 20], offs[:256], lens[:256], recs[:256], names=names,
                             check=False)
            k = int((head["ip_version"] != 0).nonzero()[0])
            a0, ver, proto = int(head["src_addr"][k, 0]), int(head["ip_version"][k]), \
                int(head["l4_proto"][k])
            pfx = f"{a0}.0.0.0/8" if ver == 4 else f"{a0:02x}00::/8"
            sel5 = (S().where("src_addr", prefix=pfx).where("dest_port", between=(1024, 49151))
                    .where("l4_proto", eq=proto).where("ip_version", eq=ver))
            t_sel5 = timed(lambda: zp.select.run(arena, offs, lens, recs, sel5, want=("idx",),
                                                 out=out, check=False))
            got = out["idx"][:int(out["count"][0])].clone()
            cols = {k2: torch.empty((n, 16) if k2 == "src_addr" else (n,), dtype=v.dtype, device=d)
                    for k2, v in head.items()}

            def composed():
                c5 = C.extract(arena, offs, lens, recs, names=names, out=cols, check=False)
                port = c5["dest_port"].to(torch.int32)
                m = (c5["src_addr"][:, 0] == a0) & (port >= 1024) & (port <= 49151) & \
                    (c5["l4_proto"] == proto) & (c5["ip_version"] == ver)
                return m.nonzero()
            t_cmp = timed(composed)
            t_ext = timed(lambda: C.extract(arena, offs, lens, recs, names=names, out=cols,
                                            check=False))
            same = torch.equal(composed().flatten(), got.long())
            say(f"5-tuple      select {fmt(t_sel5)}   extract + torch mask + nonzero {fmt(t_cmp)} "
                f"(extract alone {fmt(t_ext)})   select/composed {t_sel5[0] / t_cmp[0]:5.2f}   "
                f"faster outside the spread: {outside(t_sel5, t_cmp)}   selected "
                f"{got.numel() / n:6.1%}   same frames: {same}")
            del cols, got
        if cfg in a.gather_configs.split(","):
            for share, hi in (("1 %", 655), ("50 %", 32767), ("100 %", None)):
                selg = S(ok=True) if hi is None else S(ok=True).where("l4_checksum", between=(0, hi))
                sg = zp.select.run(arena, offs, lens, recs, selg, want=("idx", "packed_offs"),
                                   check=False)
                c, total = (int(v) for v in sg.count.tolist())
                g_out = {"arena": torch.empty(total, dtype=torch.uint8, device=d),
                         "offs": torch.empty(c, dtype=torch.int64, device=d),
                         "lens": torch.empty(c, dtype=torch.int32, device=d),
                         "records": torch.empty((c, 8), dtype=torch.uint8, device=d)}
                t_g = timed(lambda: zp.select.gather(arena, offs, lens, recs, sg, out=g_out))
                il = sg.idx[:c].long()
                src = arena[:total]

                def baseline():
                    torch.index_select(offs, 0, il)
                    torch.index_select(lens, 0, il)
                    torch.index_select(recs, 0, il)
                    return src.clone()
                t_b = timed(baseline)
                t_c = timed(lambda: src.clone())
                say(f"gather {share:>5s}  {c:9d} frames {total / 1e9:7.3f} GB   packed gather "
                    f"{fmt(t_g)} ({2 * total / t_g[0] / 1e9:6.2f} TB/s read+write)   index_select x3 + "
                    f"clone {fmt(t_b)}   clone alone {fmt(t_c)}   gather/clone "
                    f"{t_g[0] / t_c[0]:5.2f}   gather/baseline {t_g[0] / t_b[0]:5.2f}")
                del g_out, sg, il, src
        del arena, offs, lens, recs, out
        torch.cuda.empty_cache()
    if a.log:
        with open(a.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
