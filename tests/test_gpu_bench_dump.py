"""GPU: a plain `bench.py` run and its --dump-outputs files. The plain line
carries the headline and its roofline and none of the --full legs; the dump
holds the seeded sample's records and extension chains, byte for byte what
the oracle gives for the same frames of the CPU generator (so two runs, or
two builds, with the same arguments can be compared file by file)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_dumps_sampled_outputs(zp, tmp_path):
    import bench
    import oracle as orc
    n = bench.DUMP_FRAMES + 37777          # past the sample size: the sampled path
    out_dir = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2",
           "--warmup", "1", "--config", "c6", "--packets", str(n), "--dump-outputs", str(out_dir)]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    r = json.loads(lines[0])
    assert r["steps"] == 2 and r["ms_per_step"] > 0 and r["unit"] == "Mpkt/s"
    assert abs(r["value"] - n / (r["ms_per_step"] * 1e-3) / 1e6) < 0.02 * r["value"]
    for leg in ("config5", "cpu_baseline", "h2d_d2h_inclusive"):
        assert leg not in r                 # --full only
    assert "placement" not in r["roofline"] and r["roofline"]["kernel_ms_mean"] > 0

    idx = np.load(out_dir / "frame_index.npy")
    rec = np.load(out_dir / "records.npy")
    ext = np.load(out_dir / "ext.npy")
    m = bench.DUMP_FRAMES
    assert idx.dtype == np.float64 and rec.dtype == np.float32 and ext.dtype == np.float32
    assert idx.shape == (m,) and rec.shape == (m, 8) and ext.shape == (2, m, 16)
    assert sum(os.path.getsize(out_dir / f) for f in os.listdir(out_dir)) <= 64 * 10**6
    sel = idx.astype(np.int64)
    assert np.array_equal(sel, bench.dump_sample(n)) and (np.diff(sel) > 0).all()
    assert 0 <= sel[0] and sel[-1] < n

    arena, offs, lens = zp.batch.generate_host("c6", n)
    want, want_ext = orc.parse_batch(arena, offs, lens)
    want_rec = orc.pack(want, want_ext).view(np.uint8).reshape(-1, 8)[sel]
    assert np.array_equal(rec, want_rec.astype(np.float32))
    want_bytes = np.ascontiguousarray(want_ext[:, sel]).view(np.uint8).reshape(2, m, 16)
    # c6 has outer chains (inline in their records: rebuilt for the dump) beside
    # frames without one (entries unspecified on the device: zeros in the dump)
    assert want_bytes[0].any(axis=1).any() and not want_bytes[0].any(axis=1).all()
    assert np.array_equal(ext, want_bytes.astype(np.float32))
