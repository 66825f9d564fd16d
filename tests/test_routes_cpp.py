"""zp::RouteTable / zp::route (include/zero_packet.hpp):
tests/cpp/route_main.cpp prints value_of and the mask words for two tables
and both address columns over the golden packets plus generated frames; the
same lines are built here from the Python facade and tests/route_ref.py."""
import os
import subprocess

import numpy as np
import pytest

import oracle as orc
import route_ref as rref
from test_routes import GOLDEN_TABLE, NONE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "route_main.cpp")
OUT = os.path.join(ROOT, "tests", "cpp", "_build")
TABLES = [("fib", GOLDEN_TABLE), ("halves", [("0.0.0.0/1", 7), ("8000::/1", 8), ("2000::/3", 9)])]


def _build():
    import __graft_entry__ as ge
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "route_gpu")
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


def _batch(frames):
    lens = np.array([len(f) for f in frames], np.uint32)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    arena = np.frombuffer(b"".join(frames) + bytes(64), np.uint8).copy()
    return arena, offs, lens


def _text(name, by, value):
    return f"{name} {by} 0 |" + "".join(f" {v}" for v in value) + " |" + \
        "".join(f" {int(w)}" for w in rref.mask_words(value))


def test_cpp_route_program_builds(zp, golden):
    """CPU: the facade's route table compiles warning-free and links; the
    tables the program prints are not trivial on the reference."""
    assert os.path.exists(_build())
    arena, offs, lens = _batch(_frames(zp, golden))
    recs, ext = orc.parse_batch(arena, offs, lens)
    cols, packed = orc.columns(arena, offs, lens, recs), orc.pack(recs, ext)
    for name, prefixes in TABLES:
        enc = zp.routes.encode_prefixes(prefixes)
        for by in ("dest_addr", "src_addr"):
            v = rref.value_of(enc, cols, packed, by)
            assert len(set(v.tolist())) >= (8 if name == "fib" else 4), (name, by)
            assert (v == NONE).any()
    fib = zp.routes.compile_prefixes(zp.routes.encode_prefixes(GOLDEN_TABLE))
    assert [zp.routes.lookup_host(fib, a) for a in ("192.168.1.2", "11.0.0.0", "fc00:2:0:5:100::",
                                                    "3000::")] == [3, 5, 13, NONE]


@pytest.mark.gpu
def test_cpp_route_matches_python_facade(zp, golden):
    import torch
    exe = _build()
    frames = _frames(zp, golden)
    out = subprocess.run([exe], input="".join(f.hex() + "\n" for f in frames),
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    got = out.stdout.splitlines()
    arena, offs, lens = _batch(frames)
    d = torch.device("cuda:0")
    da = torch.from_numpy(arena).to(d)
    do = torch.from_numpy(offs.astype(np.int64)).to(d)
    dl = torch.from_numpy(lens.astype(np.int32)).to(d)
    dr, _ = zp.batch.parse_batch(da, do, dl)
    recs, ext = orc.parse_batch(arena, offs, lens)
    cols, packed = orc.columns(arena, offs, lens, recs), orc.pack(recs, ext)
    assert len(got) == 2 * len(TABLES) + 3
    lines = iter(got)
    for name, prefixes in TABLES:
        table = zp.routes.RouteTable(prefixes, d)
        for by in ("dest_addr", "src_addr"):
            line = next(lines)
            r = table.run(da, do, dl, dr, by=by)
            value = r.value_of.cpu().numpy().view(np.uint32)
            assert line == _text(name, by, value), (name, by, line[:200])
            assert np.array_equal(r.mask.cpu().numpy().view(np.uint64), rref.mask_words(value))
            ref = rref.value_of(table.prefixes, cols, packed, by)     # and both equal the rule
            assert line == _text(name, by, ref), (name, by)
        if name == "fib":
            assert next(lines) == f"lookup: 3 5 13 {NONE}"
    assert next(lines).startswith("refusal: zp_route_table_bytes: ") and "prefix 0: address bits" in got[-2]
    assert got[-1].startswith("refusal: zp_route_device: ") and "null status" in got[-1]
