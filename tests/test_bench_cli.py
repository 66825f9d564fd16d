"""CPU: bench.py's rank-count guard. Under a launcher, --gpus must equal
WORLD_SIZE; the check runs before anything touches the GPU, so it is
testable here."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gpus_must_match_world_size():
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "3"],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 2
    assert "WORLD_SIZE=2" in out.stderr
    assert not [l for l in out.stdout.splitlines() if l.startswith("{")]


def test_host_cores_reports_affinity():
    sys.path.insert(0, ROOT)
    import bench
    threads, visible, quota = bench.host_cores()
    assert visible == len(os.sched_getaffinity(0))
    assert 1 <= threads <= visible
    if quota is not None:
        assert threads <= max(1, int(quota))


def test_dump_sample_is_fixed_and_bounded():
    """--dump-outputs: every frame of a small batch, else the same sorted
    DUMP_FRAMES distinct indices on every call; 160 B per frame as float32
    records + ext and 8 B of index stay under 64 MB."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    assert np.array_equal(bench.dump_sample(1000), np.arange(1000))
    assert np.array_equal(bench.dump_sample(bench.DUMP_FRAMES), np.arange(bench.DUMP_FRAMES))
    a, b = bench.dump_sample(1 << 24), bench.dump_sample(1 << 24)
    assert np.array_equal(a, b) and a.dtype == np.int64 and a.shape == (bench.DUMP_FRAMES,)
    assert (np.diff(a) > 0).all() and a[0] >= 0 and a[-1] < 1 << 24
    assert bench.DUMP_FRAMES * (4 * (8 + 2 * 16) + 8) <= 64 * 10**6


def test_parse_count_suffixes():
    sys.path.insert(0, ROOT)
    import bench
    assert bench.parse_count("8M") == 8 << 20
    assert bench.parse_count("256m") == 1 << 28
    assert bench.parse_count("4096") == 4096
    assert bench.parse_count("2K") == 2048
    assert bench.parse_count(str(bench.C5_TOTAL)) == bench.C5_TOTAL
