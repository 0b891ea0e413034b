"""mtbl::Merger::scan_batch of the C++ surface (include/mtbl.hpp) on the GPU: tests/cpp/test_merger_scan.cpp
answers a query file over source files in one merge type and prints the items; they are compared
with the per-query model of tests/merger_scan_util.py, on the small overlapping sources and on the
empty-key quirk's sources, in every merge type the class has."""
import os
import subprocess

import pytest

import merger_scan_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "oxidized-mtbl_amd", "build", "test_merger_scan")
MERGES = {"concat": U.PICK["concat"], "first": U.PICK["first"], "last": U.PICK["last"], "fn": U.PICK["concat"]}


def test_cpp_merger_scan_is_built():
    """no GPU needed: the `cpp` target of the Makefile builds the binary against libmtblx.so"""
    assert os.path.exists(EXE), "build/test_merger_scan not built (make -C oxidized-mtbl_amd cpp)"
    out = subprocess.run(["nm", "-D", "--undefined-only", EXE], capture_output=True, text=True).stdout
    assert "mtblx_merge_seg_plan" in out and "mtblx_merge_seg_emit" in out and "mtblx_merge_seg_emit_reduce" in out
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=60)   # the usage error touches no device
    assert r.returncode == 1 and "usage" in r.stderr


def _hex(b):
    return b.hex() if b else "-"


def _run(tmp_path, merge, datas, qs, limits, max_blocks=64):
    """-> (items per query, served per query) as the program prints them"""
    qf = tmp_path / "queries.txt"
    qf.write_text("".join("%s %s %s %s\n" % (q[0], _hex(q[1]), _hex(q[2]) if q[0] == "range" else "-",
                                             "-" if m is None else m) for q, m in zip(qs, limits)))
    files = []
    for i, d in enumerate(datas):
        p = tmp_path / ("src%d.mtbl" % i)
        p.write_bytes(d)
        files.append(str(p))
    r = subprocess.run([EXE, merge, str(max_blocks), str(qf)] + files, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out, served = [], []
    lines = r.stdout.splitlines()
    i = 0
    while i < len(lines):
        tag, q, n, sv = lines[i].split()
        assert tag == "Q" and int(q) == len(out)
        items = [tuple(b"" if h == "-" else bytes.fromhex(h) for h in ln.split()) for ln in lines[i + 1: i + 1 + int(n)]]
        out.append(items)
        served.append(int(sv))
        i += 1 + int(n)
    assert len(out) == len(qs)
    return out, served


def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert os.path.exists(EXE), "build/test_merger_scan not built (make -C oxidized-mtbl_amd cpp)"


@pytest.mark.gpu
@pytest.mark.parametrize("merge", ["concat", "first", "last", "fn", "sum"])
def test_cpp_small_sources(oracle, tmp_path, merge):
    _gpu()
    datas, lists, qs = U.small_sources(1024, merge == "sum")
    limits = [None] * len(qs)
    want = [U.promised_groups(U.per_source(oracle, datas, q, ("small-u64" if merge == "sum" else "small", 1024))) for q in qs]
    got, served = _run(tmp_path, merge, datas, qs, limits)
    pick = U.sum_u64 if merge == "sum" else MERGES[merge]
    assert got == [U.merged(w, pick) for w in want]
    assert any(served)
    if merge == "concat":   # queries handed back to the iterators give the same items
        narrow, sv1 = _run(tmp_path, merge, datas, qs, limits, max_blocks=1)
        assert narrow == got and not all(sv1) and any(sv1)


@pytest.mark.gpu
@pytest.mark.parametrize("merge", ["concat", "first", "last", "fn"])
def test_cpp_quirk_per_query(oracle, tmp_path, merge):
    _gpu()
    import merger_model as mm
    datas = [mm.make_source(r) for r in U.QUIRK_SOURCES]
    qs = [q for q, _ in U.QUIRK_QUERIES]
    limits = [m for _, m in U.QUIRK_QUERIES]
    want = [U.cut(U.promised_groups(U.per_source(oracle, datas, q, "quirk")), m) for q, m in zip(qs, limits)]
    assert want[0] == [(b"", [b"c"])] and want[4] == [] and want[5] == [(b"k1", [b"x", b"y"])]
    got, served = _run(tmp_path, merge, datas, qs, limits)
    assert got == [U.merged(w, MERGES[merge]) for w in want]
    assert all(served)
