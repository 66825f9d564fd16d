"""Times the header rewrite (zp_rewrite_columns_device) beside the extract of
the same columns and the parse of the same arena, in one process.

    python tools/rewrite_bench.py --config c3 [--packets 16777216] [--reps 20]
                                  [--probe] [--log profiles/rewrite_bench_c3.log]

Two column sets: NAT (src/dest address, src/dest port, TTL) and all 14
writable columns. HIP events, median of --reps repetitions after warm-up. The
repetitions alternate between random column values and the extracted original
ones, so every repetition changes every applied field and both checksums (a
rewrite of values already in the frame would skip the checksum stores).
--probe also times tools/probes/rewrite_global.hip (old words by plain global
loads instead of the cooperative staging).
"""
import argparse
import ctypes
import importlib
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NAT = ("src_addr", "dest_addr", "src_port", "dest_port", "ttl")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--packets", type=int, default=1 << 24)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--probe", action="store_true")
    ap.add_argument("--log", default="")
    a = ap.parse_args()
    zp = importlib.import_module("zero-packet_amd")
    C = zp.columns
    lib = zp._lib.hip()
    probe = None
    if a.probe:
        so = os.path.join(ROOT, "tools", "probes", "librewrite_global.so")
        src = os.path.join(ROOT, "tools", "probes", "rewrite_global.hip")
        if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
            subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17",
                            "-shared", "-fPIC", "-o", so, src], check=True)
        probe = ctypes.CDLL(so).rewrite_global
        probe.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_uint64] + [ctypes.c_void_p] * 2
    d = torch.device("cuda:0")
    n = a.packets
    s = torch.cuda.current_stream(d)
    arena, offs, lens = zp.batch.generate(a.config, n, device=d)
    recs, ext = zp.batch.parse_batch(arena, offs, lens)
    torch.cuda.synchronize()
    lines = [f"rewrite_bench {a.config}: {n} frames, {arena.numel() / 1e9:.2f} GB arena, "
             f"{torch.cuda.get_device_name(d)}, median of {a.reps}"]

    def timed(fn, reps=a.reps):
        for k in range(3):
            fn(k)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
              for _ in range(reps)]
        for k, (x, y) in enumerate(ev):
            x.record(s)
            fn(k + 3)
            y.record(s)
        torch.cuda.synchronize()
        return float(np.median([x.elapsed_time(y) for x, y in ev]))

    def ptrs(cols):
        p = (ctypes.c_void_p * len(C.COLUMNS))()
        for name, t in cols.items():
            p[C.INDEX[name]] = t.data_ptr()
        return p

    args = (arena.data_ptr(), offs.data_ptr(), lens.data_ptr())
    t_parse = timed(lambda k: lib.zp_parse_batch_device(*args, n, recs.data_ptr(), ext.data_ptr(),
                                                        s.cuda_stream))
    lines.append(f"parse                      {t_parse:8.3f} ms")
    for label, names in (("NAT (5 columns)", NAT), ("all 14 columns", C.WRITABLE)):
        orig = C.extract(arena, offs, lens, recs, names=list(names), check=False)
        rnd = {k: torch.randint(0, 256, (t.numel() * t.element_size(),), dtype=torch.uint8,
                                device=d).view(t.dtype).view(t.shape) for k, t in orig.items()}
        out = {k: torch.empty_like(t) for k, t in orig.items()}
        sets = [ptrs(rnd), ptrs(orig)]
        po = ptrs(out)
        t_ext = timed(lambda k: lib.zp_extract_columns_device(*args, recs.data_ptr(), n, po,
                                                              s.cuda_stream))
        t_rw = timed(lambda k: lib.zp_rewrite_columns_device(*args, recs.data_ptr(), n,
                                                             sets[k & 1], s.cuda_stream),
                     reps=a.reps | 1)
        # reps | 1 and three warm-up runs: an even number of rewrites in all,
        # so the arena holds the original values again
        lines.append(f"{label:16s} extract {t_ext:8.3f} ms   rewrite {t_rw:8.3f} ms   "
                     f"rewrite/extract {t_rw / t_ext:5.2f}   rewrite/parse {t_rw / t_parse:5.2f}   "
                     f"{n / t_rw / 1e6:7.2f} G frames/s")
        if probe is not None:
            t_gl = timed(lambda k: probe(*args, recs.data_ptr(), n, sets[k & 1], s.cuda_stream),
                         reps=a.reps | 1)
            lines.append(f"{label:16s} global-load probe   rewrite {t_gl:8.3f} ms   "
                         f"probe/staged {t_gl / t_rw:5.2f}")
        r2, _ = zp.batch.parse_batch(arena, offs, lens, check=False)
        back = C.extract(arena, offs, lens, r2, names=list(names), check=False)
        torch.cuda.synchronize()
        ok = torch.equal(r2, recs) and all(torch.equal(back[k], orig[k]) for k in orig)
        lines.append(f"{label:16s} records unchanged and original values restored: {ok}")
        del orig, rnd, out, back
    text = "\n".join(lines)
    print(text, flush=True)
    if a.log:
        with open(a.log, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
