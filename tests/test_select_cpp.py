"""zp::Select / zp::select / zp::gather_frames (include/zero_packet.hpp):
tests/cpp/select_main.cpp prints count, idx and the packed bytes for three
selectors over the golden packets plus generated frames; the same lines are
built here from the Python facade and tests/select_ref.py."""
import os
import subprocess

import numpy as np
import pytest

import oracle as orc
import select_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "select_main.cpp")
OUT = os.path.join(ROOT, "tests", "cpp", "_build")


def _build():
    import __graft_entry__ as ge
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "select_gpu")
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
    return frames + [arena[o:o + l].tobytes() for o, l in zip(offs, lens)]


def test_cpp_select_program_builds(zp, golden):
    """CPU: the facade's selector compiles warning-free and links."""
    assert os.path.exists(_build())


@pytest.mark.gpu
def test_cpp_select_matches_python_facade(zp, golden):
    import torch
    exe = _build()
    frames = _frames(zp, golden)
    out = subprocess.run([exe], input="".join(f.hex() + "\n" for f in frames),
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    got = out.stdout.splitlines()
    # the same batch (frames back to back) through the Python facade
    lens = np.array([len(f) for f in frames], np.uint32)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    arena = np.frombuffer(b"".join(frames) + bytes(64), np.uint8).copy()
    d = torch.device("cuda:0")
    da = torch.from_numpy(arena).to(d)
    do = torch.from_numpy(offs.astype(np.int64)).to(d)
    dl = torch.from_numpy(lens.astype(np.int32)).to(d)
    dr, _ = zp.batch.parse_batch(da, do, dl)
    S, R = zp.select.Select, zp.records
    sels = [("tcp", S(ok=True, has=("tcp",))),
            ("five", S(ok=True).where("l4_proto", eq=17).where("dest_port", between=(1000, 40000))
             .where("src_addr", prefix="192.168.0.0/16").where("ip_version", eq=4)),
            ("v6", S(min_len=70).where("ttl", outside=(0, 63)).where("dest_addr", prefix="fe80::/10")
             .where("src_mac", mac="34:97:f6:94:02:0f"))]
    recs, ext = orc.parse_batch(arena, offs, lens)
    cols, packed = orc.columns(arena, offs, lens, recs), orc.pack(recs, ext)
    assert len(got) == len(sels) + 1
    for line, (name, sel) in zip(got, sels):
        s = zp.select.run(da, do, dl, dr, sel, want=("idx", "packed_offs"))
        a2, *_ = zp.select.gather(da, do, dl, dr, s)
        c, total = s.count.tolist()
        idx = s.idx.cpu().numpy()[:c]
        want = f"{name} {c} {total} |" + "".join(f" {i}" for i in idx) + " | " + \
            a2.cpu().numpy().tobytes().hex()
        assert line == want, (name, line[:200], want[:200])
        m = ref.select_mask(sel.encode(), cols, packed, lens)          # and both equal the rule
        assert np.array_equal(idx.astype(np.uint32), np.flatnonzero(m)) and c > 0, name
    assert got[-1].startswith("refusal: zp_select_device: ") and "null count" in got[-1]
