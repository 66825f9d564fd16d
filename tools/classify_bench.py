"""Times the rule table (zp_classify_device) beside what a caller writes
without it, on the same frames in one process.

    python tools/classify_bench.py [--configs c3,c4] [--packets 16777216] [--rules 1,4,16,64,256]
                                   [--reps 5] [--runs 5] [--log profiles/classify_bench.log]

Rules (fixed seed): rule r is a five-tuple selector: a /4 source prefix, a
dest-port range 16,384 ports wide, l4_proto 6 or 17 and the config's
ip_version. Addresses and ports of the generated configs are uniform, so one
rule takes about 1 / 192 of the frames and the share no rule takes falls with
R; each row states it as measured.
Rows per config and R (HIP events; each run is the median of --reps
repetitions after warm-up, a row reports the median of --runs runs and their
min-max):
  classify   RuleTable.run(check=False): rule_of, hits and mask in one launch
  baseline   R calls of select.run(want=("mask",), check=False), the R masks
             combined into rule_of in torch (first set bit by priority), and
             scatter_add of ones and lens into the R + 1 counters; its three
             parts are also timed apart. Results must equal classify's.
Then classify at R = 1 beside select of the same rule, a hot-rule table (every
frame matches rule 0) and a record-only table (no frame is read).
"""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_rules(zp, cfg, count, seed=20240521):
    S = zp.select.Select
    rng = np.random.default_rng(seed)
    v6 = cfg in ("c4",)
    rules = []
    for _ in range(count):
        nib = int(rng.integers(0, 16)) << 4
        lo = int(rng.integers(0, 65536 - 16384))
        proto = int(rng.choice([6, 17]))
        prefix = f"{nib:02x}00::/4" if v6 else f"{nib}.0.0.0/4"
        rules.append(S().where("src_addr", prefix=prefix).where("dest_port", between=(lo, lo + 16383))
                     .where("l4_proto", eq=proto).where("ip_version", eq=6 if v6 else 4))
    return rules


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c3,c4")
    ap.add_argument("--packets", type=int, default=1 << 24)
    ap.add_argument("--rules", default="1,4,16,64,256")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--log", default="")
    a = ap.parse_args()
    zp = importlib.import_module("zero-packet_amd")
    lib = zp._lib.hip()
    d = torch.device("cuda:0")
    n = a.packets
    s = torch.cuda.current_stream(d)
    counts = [int(x) for x in a.rules.split(",")]
    lines = []

    def say(x):
        print(x, flush=True)
        lines.append(x)
    say(f"classify_bench: {n} frames, {torch.cuda.get_device_name(d)}, per row the median of {a.runs} "
        f"runs (each the median of {a.reps} repetitions) and the runs' min-max")

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

    words = (n + 63) // 64
    shifts = torch.arange(8, dtype=torch.uint8, device=d)
    for cfg in [c for c in a.configs.split(",") if c]:
        arena, offs, lens = zp.batch.generate(cfg, n, device=d)
        recs, _ = zp.batch.parse_batch(arena, offs, lens)
        torch.cuda.synchronize()
        say(f"--- {cfg}: {arena.numel() / 1e9:.2f} GB arena, {arena.numel() / n:.0f} B per frame")
        lens64 = lens.to(torch.int64)
        ones = torch.ones(n, dtype=torch.int64, device=d)
        out = {"rule_of": torch.empty(n, dtype=torch.int32, device=d),
               "mask": torch.empty(words, dtype=torch.int64, device=d),
               "status": torch.zeros(1, dtype=torch.int64, device=d)}
        sel_out = {"count": torch.zeros(2, dtype=torch.int64, device=d),
                   "scratch": torch.empty(int(lib.zp_select_scratch_bytes(n)), dtype=torch.uint8,
                                          device=d)}
        all_rules = make_rules(zp, cfg, max(counts))
        t_cls, t_base = {}, {}
        for R in counts:
            rules = all_rules[:R]
            table = zp.classify.RuleTable(rules, d)
            t_cls[R] = timed(lambda: table.run(arena, offs, lens, recs, out=out, check=False))
            table.reset_hits()
            table.run(arena, offs, lens, recs, out=out, check=False)
            torch.cuda.synchronize()
            assert int(out["status"][0]) == 0
            got_rule, got_hits = out["rule_of"].clone(), table.hits.clone()
            none = float((got_rule < 0).sum()) / n
            t_rule = timed(lambda: table.run(arena, offs, lens, recs, want=("rule_of",), out=out,
                                             check=False))
            # the baseline: R select passes, a torch combine, scatter_add
            masks = torch.empty((R, words), dtype=torch.int64, device=d)
            base_rule = torch.empty(n, dtype=torch.int32, device=d)
            base_hits = torch.zeros((R + 1, 2), dtype=torch.int64, device=d)

            def passes():
                for r in range(R):
                    zp.select.run(arena, offs, lens, recs, rules[r], want=("mask",),
                                  out={"mask": masks[r], **sel_out}, check=False)

            def combine():
                base_rule.fill_(-1)
                for r in range(R - 1, -1, -1):
                    bits = ((masks[r].view(torch.uint8).unsqueeze(1) >> shifts) & 1).view(-1)[:n]
                    base_rule.masked_fill_(bits.bool(), r)

            def count():
                slot = torch.where(base_rule < 0, R, base_rule).to(torch.int64)
                base_hits.zero_()
                base_hits[:, 0].scatter_add_(0, slot, ones)
                base_hits[:, 1].scatter_add_(0, slot, lens64)

            def baseline():
                passes()
                combine()
                count()
            slow = R >= 64
            kw = dict(reps=2 if slow else a.reps, runs=3 if slow else a.runs)
            t_base[R] = timed(baseline, **kw)
            t_p, t_c, t_s = timed(passes, **kw), timed(combine, **kw), timed(count, **kw)
            same = torch.equal(base_rule, got_rule) and torch.equal(base_hits, got_hits)
            say(f"{cfg} R={R:<4d} classify {fmt(t_cls[R])}  rule_of only {t_rule[0]:8.3f} ms   "
                f"{n / t_cls[R][0] / 1e6:6.2f} Gframes/s   no rule {100 * none:5.1f} %")
            say(f"{cfg} R={R:<4d} baseline {fmt(t_base[R])}{' (3 runs of 2)' if slow else ''}  = select "
                f"passes {t_p[0]:.3f} + combine {t_c[0]:.3f} + scatter_add {t_s[0]:.3f}   "
                f"baseline/classify {t_base[R][0] / t_cls[R][0]:7.2f}   faster outside the spread: "
                f"{'yes' if t_cls[R][2] < t_base[R][1] else 'no'}   same rule_of and hits: {same}")
            if R == 1:
                t_sel = timed(lambda: zp.select.run(arena, offs, lens, recs, rules[0], want=("mask",),
                                                    out={"mask": masks[0], **sel_out}, check=False))
                t_m = timed(lambda: table.run(arena, offs, lens, recs, want=("mask",), out=out,
                                              check=False))
                say(f"{cfg} R=1    select of the same rule (mask only) {fmt(t_sel)}   classify (mask "
                    f"only) {fmt(t_m)}   classify/select {t_m[0] / t_sel[0]:5.2f}   classify (all "
                    f"three)/select {t_cls[1][0] / t_sel[0]:5.2f}")
            del masks, base_rule, got_rule
        wins = [R for R in counts if t_cls[R][2] < t_base[R][1]]
        per = [(t_cls[b][0] - t_cls[a_][0]) / (b - a_) * 1e3 for a_, b in zip(counts, counts[1:])]
        say(f"{cfg} smallest R at which classify wins outside the spread: {min(wins) if wins else 'none'}"
            f"   time per added rule: " + ", ".join(
                f"{a_}->{b}: {p:.1f} us" for (a_, b), p in zip(zip(counts, counts[1:]), per)))
        # every frame matches rule 0: all counters of a tile go to one entry
        S = zp.select.Select
        hot = zp.classify.RuleTable([S().where("ttl", between=(0, 255))] + all_rules[:15], d)
        t_hot = timed(lambda: hot.run(arena, offs, lens, recs, out=out, check=False))
        hot.reset_hits()
        hot.run(arena, offs, lens, recs, out=out, check=False)
        h = hot.hits_numpy()
        say(f"{cfg} hot rule (16 rules, every frame matches rule 0) {fmt(t_hot)}   hits[0] "
            f"{int(h['packets'][0])} packets {int(h['bytes'][0])} bytes, equal to n and sum(lens): "
            f"{int(h['packets'][0]) == n and int(h['bytes'][0]) == int(lens64.sum())}")
        rec = zp.classify.RuleTable([S(has=("tcp",), min_len=200), S(has=("udp",)), S(ok=False),
                                     S(any_of=("icmpv4", "icmpv6"))], d)
        t_rec = timed(lambda: rec.run(None, None, lens, recs, out=out, check=False))
        t_recsel = timed(lambda: zp.select.run(None, None, lens, recs, S(has=("udp",)), want=("mask",),
                                               out={"mask": out["mask"], **sel_out}, check=False))
        say(f"{cfg} record-only table (4 rules, no frame read) {fmt(t_rec)}   one record-only select "
            f"{fmt(t_recsel)}")
        del arena, offs, lens, recs, lens64, ones, out, sel_out
        torch.cuda.empty_cache()
    if a.log:
        with open(a.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
