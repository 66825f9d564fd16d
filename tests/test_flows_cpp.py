"""zp::FlowOpts / zp::flow_aggregate (include/zero_packet.hpp):
tests/cpp/flow_main.cpp prints count, flow_of and the flow entries for three
option sets over the golden packets plus generated frames; the same lines are
built here from the Python facade and tests/flow_ref.py."""
import os
import subprocess

import numpy as np
import pytest

import flow_ref as ref
import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "flow_main.cpp")
OUT = os.path.join(ROOT, "tests", "cpp", "_build")


def _build():
    import __graft_entry__ as ge
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "flow_gpu")
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
    return frames + gen + gen[:150] + frames               # flows of several frames


def test_cpp_flow_program_builds(zp, golden):
    """CPU: the facade's flow entry point compiles warning-free and links."""
    assert os.path.exists(_build())


@pytest.mark.gpu
def test_cpp_flows_match_python_facade(zp, golden):
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
    n = len(frames)
    d = torch.device("cuda:0")
    da = torch.from_numpy(arena).to(d)
    do = torch.from_numpy(offs.astype(np.int64)).to(d)
    dl = torch.from_numpy(lens.astype(np.int32)).to(d)
    dr, _ = zp.batch.parse_batch(da, do, dl)
    recs, ext = orc.parse_batch(arena, offs, lens)
    cols, packed = orc.columns(arena, offs, lens, recs), orc.pack(recs, ext)
    sets = [("five", dict()), ("bidir", dict(bidir=True, vlan=True)),
            ("addr", dict(ports=False, proto=False, hash_mask=3))]
    want = []
    for name, kw in sets:
        t = zp.flows.aggregate(da, do, dl, dr, **kw)
        count = [int(v) for v in t.count.tolist()]
        ent = zp.flows.to_numpy(t)
        fo = t.flow_of.cpu().numpy().view(np.uint32)
        want.append(f"{name} {count[0]} {count[1]} {count[2]} {count[3]} |" +
                    "".join(f" {f}" for f in fo))
        want += [e.tobytes().hex() for e in ent]
        flags = zp.flows.key_flags(**{k: v for k, v in kw.items() if k != "hash_mask"})
        wfo, went, wcnt = ref.aggregate(cols, packed, lens, zp.flows.encode_opts(flags, n))
        assert count == wcnt and np.array_equal(fo, wfo) and ent.tobytes() == went.tobytes(), name
        assert 10 < count[0] < count[1] < n, name           # and both equal the rule
    assert got[:-1] == want, [(a[:120], b[:120]) for a, b in zip(got, want) if a != b][:2]
    assert got[-1].startswith("refusal: zp_flow_aggregate_device: ") and "max_flows" in got[-1]
