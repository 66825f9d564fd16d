"""zp::RuleTable / zp::classify (include/zero_packet.hpp):
tests/cpp/classify_main.cpp prints rule_of and hits for three tables over the
golden packets plus generated frames; the same lines are built here from the
Python facade and tests/classify_ref.py."""
import os
import subprocess

import numpy as np
import pytest

import classify_ref as cref
import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "classify_main.cpp")
OUT = os.path.join(ROOT, "tests", "cpp", "_build")


def _build():
    import __graft_entry__ as ge
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "classify_gpu")
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


def _tables(zp):
    S = zp.select.Select
    return [("acl", [S(ok=True, has=("tcp",)).where("dest_port", eq=43424),
                     S(ok=True).where("l4_proto", eq=17).where("dest_port", between=(1000, 40000))
                     .where("src_addr", prefix="192.168.0.0/16").where("ip_version", eq=4),
                     S(min_len=70).where("ttl", outside=(0, 63)).where("dest_addr", prefix="fe80::/10"),
                     S(ok=True, has=("tcp",)), S(ok=False)]),
            ("records", [S(has=("tcp",)), S(has=("udp",), max_len=120), S(ok=False)]),
            ("nested", [S().where("src_port", between=((69 - r) * 936, 65535)) for r in range(70)])]


def _batch(frames):
    lens = np.array([len(f) for f in frames], np.uint32)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    arena = np.frombuffer(b"".join(frames) + bytes(64), np.uint8).copy()
    return arena, offs, lens


def test_cpp_classify_program_builds(zp, golden):
    """CPU: the facade's rule table compiles warning-free and links; the
    tables the program prints are not trivial on the reference."""
    assert os.path.exists(_build())
    arena, offs, lens = _batch(_frames(zp, golden))
    recs, ext = orc.parse_batch(arena, offs, lens)
    cols, packed = orc.columns(arena, offs, lens, recs), orc.pack(recs, ext)
    for name, rules in _tables(zp):
        r = cref.rule_of(zp.classify.encode_rules(rules), cols, packed, lens)
        assert len(set(r.tolist())) >= (20 if name == "nested" else 4), name


@pytest.mark.gpu
def test_cpp_classify_matches_python_facade(zp, golden):
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
    tables = _tables(zp)
    assert len(got) == len(tables) + 1

    def text(name, frames_needed, rule, hits):
        return f"{name} {int(frames_needed)} 0 |" + "".join(f" {r}" for r in rule) + " |" + \
            "".join(f" {int(p)}:{int(b)}" for p, b in zip(hits["packets"], hits["bytes"]))
    for line, (name, rules) in zip(got, tables):
        table = zp.classify.RuleTable(rules, d)
        c = table.run(da, do, dl, dr, want=("rule_of", "hits"))
        rule = c.rule_of.cpu().numpy().view(np.uint32)
        assert line == text(name, table.needs_frames, rule, table.hits_numpy()), (name, line[:200])
        ref = cref.rule_of(table.rules, cols, packed, lens)            # and both equal the rule
        assert line == text(name, name != "records", ref, cref.hits(ref, lens, table.nrules)), name
    assert got[-1].startswith("refusal: zp_classify_device: ") and "null status" in got[-1]
