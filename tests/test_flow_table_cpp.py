"""zp::FlowTable (include/zero_packet.hpp): tests/cpp/flow_table_main.cpp runs
two updates and one retire over the golden packets plus generated frames and
prints the counts, flow_of, remap and the entries; the same lines are built
here from the Python facade and tests/flow_table_ref.py."""
import os
import subprocess

import numpy as np
import pytest

import flow_ref as ref
import flow_table_ref as tref
import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "flow_table_main.cpp")
OUT = os.path.join(ROOT, "tests", "cpp", "_build")


def _build():
    import __graft_entry__ as ge
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "flow_table_gpu")
    deps = [SRC, os.path.join(ROOT, "include", "zero_packet.hpp"),
            os.path.join(ROOT, "include", "zero_packet.h")]
    if os.path.exists(exe) and all(os.path.getmtime(exe) > os.path.getmtime(d) for d in deps):
        return exe
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(ge.HIPCC)))
    lib = os.path.join(ROOT, "zero-packet_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror",
                    "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
                    "-isystem", os.path.join(rocm, "include"), "-o", exe, SRC, "-L" + lib,
                    "-lzp_hip", "-L" + os.path.join(rocm, "lib"), "-lamdhip64",
                    "-Wl,-rpath," + lib, "-Wl,-rpath," + os.path.join(rocm, "lib")], check=True)
    return exe


def _frames(zp, golden):
    frames = [bytes.fromhex(fx["bytes"]) for fx in golden["fixtures"]]
    arena, offs, lens = zp.batch.generate_host("c5", 300, first=31)
    gen = [arena[o:o + l].tobytes() for o, l in zip(offs, lens)]
    return frames + gen + gen[:150] + frames               # flows of several frames, in both updates


def _batch(frames):
    lens = np.array([len(f) for f in frames], np.uint32)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    arena = np.frombuffer(b"".join(frames) + bytes(64), np.uint8).copy()
    return arena, offs, lens


def _reference(zp, golden):
    """The lines the program must print, by flow_table_ref, and the batch."""
    frames = _frames(zp, golden)
    arena, offs, lens = _batch(frames)
    n = len(frames)
    recs, ext = orc.parse_batch(arena, offs, lens)
    cols, packed = orc.columns(arena, offs, lens, recs), orc.pack(recs, ext)
    rt = tref.Table(zp.flows.encode_opts(zp.flows.key_flags(bidir=True), n))
    want, counts = [], []
    for lo, hi in ((0, n // 3), (n // 3, n)):
        fo, cnt = rt.update({k: v[lo:hi] for k, v in cols.items()}, packed[lo:hi], lens[lo:hi])
        want.append("update " + " ".join(str(c) for c in cnt) + " |" + "".join(f" {f}" for f in fo))
        counts.append(cnt)
    gone, remap, rc = rt.retire(1, 0x05)
    want.append(f"retire {rc[0]} {rc[1]} |" + "".join(f" {f}" for f in remap))
    want += [e.tobytes().hex() for e in gone] + [e.tobytes().hex() for e in rt.states()]
    return frames, (arena, offs, lens), want, counts, rc


def test_cpp_flow_table_program_builds(zp, golden):
    """CPU: the facade's table class compiles warning-free and links; and the
    program's input does what the GPU test needs of it."""
    assert os.path.exists(_build())
    _, _, _, counts, rc = _reference(zp, golden)
    assert counts[0][1] > 10 and counts[1][1] > 10 and counts[1][2] - counts[1][1] > 100, "hits and new keys"
    assert rc[0] > 10 and rc[1] > 10, "the retire keeps some flows and retires some"


@pytest.mark.gpu
def test_cpp_flow_table_matches_python_facade(zp, golden):
    import torch
    exe = _build()
    frames, (arena, offs, lens), want, _, _ = _reference(zp, golden)
    out = subprocess.run([exe], input="".join(f.hex() + "\n" for f in frames),
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    got = out.stdout.splitlines()
    assert got[:-1] == want, [(a[:120], b[:120]) for a, b in zip(got, want) if a != b][:2]
    assert got[-1].startswith("refusal: zp_flow_table_init_device: ") and "table_bytes" in got[-1]
    # the same through the Python facade
    n = len(frames)
    d = torch.device("cuda:0")
    da = torch.from_numpy(arena).to(d)
    do = torch.from_numpy(offs.astype(np.int64)).to(d)
    dl = torch.from_numpy(lens.astype(np.int32)).to(d)
    dr, _ = zp.batch.parse_batch(da, do, dl)
    t = zp.flows.Table(n, d, bidir=True)
    mine = []
    for lo, hi in ((0, n // 3), (n // 3, n)):
        u = t.update(da, do[lo:hi], dl[lo:hi], dr[lo:hi])
        mine.append("update " + " ".join(str(int(c)) for c in u.count.tolist()) + " |" +
                    "".join(f" {f}" for f in u.flow_of.cpu().numpy().view(np.uint32)))
    f_old = int(u.count[0])
    r = t.retire(max_idle=1, tcp_any=0x05)
    f1, k = (int(v) for v in r.count.tolist())
    mine.append(f"retire {f1} {k} |" + "".join(f" {f}" for f in r.remap.cpu().numpy().view(np.uint32)[:f_old]))
    mine += [e.tobytes().hex() for e in r.retired.cpu().numpy()[:k].reshape(-1).view(tref.STATE_DTYPE)]
    mine += [e.tobytes().hex() for e in t.to_numpy()]
    assert mine == want and ref.NONE == zp.flows.FLOW_NONE
