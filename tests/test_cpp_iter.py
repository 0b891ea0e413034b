"""The C++ Reader and its iterators (include/mtbl.hpp: Reader, ReaderIntoIter, Reader::get, len,
scan_batch) against the oracle, script for script.

tests/cpp/iter_driver.cpp (build/iter_driver) opens one file and runs a script of commands through
the public API of mtbl.hpp; every outcome, op count and record it writes is compared with
pyoracle.file_scan / pyoracle.iter_script -- never with the Python mtblx.reader.  The files, seeds
and comparison rules are those of tests/test_seek_gpu.py and tests/test_scan_batch_gpu.py.

Oracle outcome -> C++ outcome (the header's contract): END_NONE -> a clean end with equal ops;
END_ERR_OPEN -> mtbl::Error at open or construction with the oracle's name; Err in next -> op code
2 and the same name; END_PANIC and END_LOOP -> mtbl::Panic after exactly the oracle's records.

A "case" is one file and one driver run.  The corpus conditions (which keep the corrupt and
irregular cases from passing vacuously) are checked with the oracle alone in the non-gpu tests at
the end, per group of cases: the corrupt-data files together, and the six damaged copies of each
index damage kind together.  Where the seeds of test_seek_gpu.py miss a condition, the first later
seed that meets them all is used (FLIP_SEED, IRREGULAR_SEED)."""
import bisect
import functools
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import corpus
import scan_util as su
import test_seek_gpu as ts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "oxidized-mtbl_amd", "build", "iter_driver")
END_NONE, END_ERR_OPEN, END_ERR_NEXT, END_PANIC, END_LOOP = range(5)
MODE_ID = {"iter": 0, "from": 1, "prefix": 2, "range": 3}
KIND_ID = {"from": 0, "get": 1, "prefix": 2, "range": 3}


# ---------------------------------------------------------------- commands: encode / parse / expect
# ("open", verify) | ("iter", mode, key, key2, ops) | ("scan", mode, key, key2, max_records)
# | ("get", key) | ("len",) | ("scan_batch", max_blocks, queries, limits, tag)
def _b(x):
    return struct.pack("<I", len(x)) + x


def encode(cmds):
    out = []
    for c in cmds:
        if c[0] == "open":
            out.append(b"O" + bytes([1 if c[1] else 0]))
        elif c[0] == "iter":
            out.append(b"I" + bytes([MODE_ID[c[1]]]) + _b(c[2]) + _b(c[3]) + struct.pack("<I", len(c[4])))
            for op in c[4]:
                out.append(b"\0" + struct.pack("<Q", op) if isinstance(op, int) else b"\1" + _b(op[1]))
        elif c[0] == "scan":
            out.append(b"S" + bytes([MODE_ID[c[1]]]) + _b(c[2]) + _b(c[3]) + struct.pack("<Q", c[4]))
        elif c[0] == "get":
            out.append(b"G" + _b(c[1]))
        elif c[0] == "len":
            out.append(b"L")
        else:
            out.append(b"B" + struct.pack("<II", c[1], len(c[2])))
            for q, m in zip(c[2], c[3]):
                out.append(bytes([KIND_ID[q[0]]]) + _b(q[1]) + _b(q[2] if q[0] == "range" else b"") +
                           struct.pack("<BQ", m is not None, m or 0))
    return b"".join(out)


class _Cursor:
    def __init__(self, data):
        self.d, self.p = data, 0

    def take(self, fmt):
        v = struct.unpack_from(fmt, self.d, self.p)
        self.p += struct.calcsize(fmt)
        return v if len(v) > 1 else v[0]

    def bytes(self):
        n = self.take("<I")
        self.p += n
        assert self.p <= len(self.d), "driver output truncated"
        return self.d[self.p - n: self.p]

    def records(self):
        return [(self.bytes(), self.bytes()) for _ in range(self.take("<Q"))]


def parse_one(cur, cmd):
    """the driver's result of one command -> dict"""
    tag = {"open": b"O", "iter": b"I", "scan": b"S", "get": b"G", "len": b"L", "scan_batch": b"B"}[cmd[0]]
    assert cur.d[cur.p: cur.p + 1] == tag, "driver output out of step"
    cur.p += 1
    code = cur.take("<B")
    err = cur.bytes().decode()
    r = dict(code=code, err=err)
    if cmd[0] == "iter":
        r["ops"] = [cur.take("<QB") for _ in range(cur.take("<I"))]
        r["records"] = cur.records()
    elif cmd[0] == "scan":
        r["records"] = cur.records()
    elif cmd[0] == "get" and code < 2:
        r["value"] = cur.bytes()
    elif cmd[0] == "len" and code == 0:
        r["len"] = cur.take("<Q")
    elif cmd[0] == "scan_batch" and code == 0:
        nq = cur.take("<I")
        r["queries"] = [cur.records() for _ in range(nq)]
        r["served"] = list(cur.d[cur.p: cur.p + nq])
        cur.p += nq
    return r


def expect_one(oracle, data, verify, cmd):
    """the oracle's side of one command"""
    if cmd[0] == "iter":
        return oracle.iter_script(data, cmd[1], cmd[2], cmd[3], cmd[4], verify=verify)
    if cmd[0] == "scan":
        return oracle.file_scan(data, cmd[1], cmd[2], cmd[3], verify=verify, max_records=cmd[4])
    if cmd[0] == "get":
        return oracle.file_scan(data, "get", cmd[1], verify=verify)
    if cmd[0] == "len":
        return oracle.file_scan(data, "iter", verify=verify)
    if cmd[0] == "scan_batch":
        return [su.expected(oracle, data, q, m, verify, tag=cmd[4]) for q, m in zip(cmd[2], cmd[3])]
    return None


def _end_of(exp):
    """oracle end -> driver end (END_LOOP is a Panic in the header)"""
    return END_PANIC if exp["end"] == END_LOOP else exp["end"]


def _short(x):
    """a command for an assertion message: long keys cut"""
    if isinstance(x, (bytes, bytearray)):
        return bytes(x[:24]) + b"...(%d)" % len(x) if len(x) > 32 else bytes(x)
    if isinstance(x, (tuple, list)):
        return tuple(_short(y) for y in x[:12])
    return x


def compare_one(cmd, got, exp):
    what = _short(cmd)
    if cmd[0] == "iter":
        assert got["code"] == _end_of(exp), (what, got["code"], exp["end"])
        assert got["records"] == exp["records"], (what, len(got["records"]), len(exp["records"]))
        nops = len(got["ops"])
        assert got["ops"] == exp["ops"][:nops], (got["ops"], exp["ops"])
        if exp["end"] == END_NONE:
            assert nops == len(exp["ops"])
            if any(c == 2 for _, c in exp["ops"]):
                assert got["err"] == exp["err"]
        elif exp["end"] == END_ERR_OPEN:
            assert got["err"] == exp["err"]
    elif cmd[0] == "scan":
        errs = (END_ERR_OPEN, END_ERR_NEXT)
        assert (got["code"], got["err"] if got["code"] in errs else None) == \
            (_end_of(exp), exp["err"] if exp["end"] in errs else None), what
        assert got["records"] == exp["records"], (what, len(got["records"]), len(exp["records"]))
    elif cmd[0] == "get":
        if exp["end"] == END_NONE:      # Reader::get's value: the found record's, or the held one after Some(Err)
            want = (0, exp["records"][0][1]) if exp["records"] else (1, b"")
            assert (got["code"], got.get("value")) == want, what
        elif exp["end"] == END_ERR_OPEN:
            assert (got["code"], got["err"]) == (2, exp["err"]), what
        else:
            assert exp["end"] in (END_PANIC, END_LOOP) and got["code"] == 3, (what, exp["end"], got["code"])
    elif cmd[0] == "len":
        if got["code"] == 0:
            assert got["len"] == len(exp["records"])
        else:                           # the open itself failed: the oracle's scan ends there too
            assert not exp["records"] and (got["code"], exp["end"]) in ((2, END_ERR_OPEN), (3, END_PANIC))
    elif cmd[0] == "scan_batch":
        assert got["code"] == 0, got
        assert len(got["queries"]) == len(exp)
        for q, g, e in zip(cmd[2], got["queries"], exp):
            assert e["end"] == END_NONE
            assert g == e["records"], (_short(q), len(g), len(e["records"]))


def expect_all(oracle, data, cmds):
    verify, out = True, []
    for c in cmds:
        if c[0] == "open":
            verify = c[1]
        out.append(expect_one(oracle, data, verify, c))
    return out


def _keep(data, *what):
    """keep the offending file as test_seek_gpu does (the case builders rebuild its script)"""
    ts._dump_failure(data, *what)


def run_case(oracle, tmp_path, data, cmds):
    """one driver run over one file; every command compared with the oracle -> (results, expected)"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert os.path.exists(EXE), "build/iter_driver not built (make -C oxidized-mtbl_amd cpp)"
    exp = expect_all(oracle, data, cmds)
    f, s, o = (str(tmp_path / n) for n in ("file.mtbl", "script.bin", "out.bin"))
    open(f, "wb").write(data)
    open(s, "wb").write(encode(cmds))
    try:
        r = subprocess.run([EXE, f, s, o], capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        _keep(data, "iter_driver", "timeout")
        pytest.exit("iter_driver hung: nothing more is started on this device", returncode=3)
    if r.returncode != 0:
        _keep(data, "iter_driver", r.returncode, r.stderr[-2000:])
    if r.returncode < 0 or r.returncode > 2 or "illegal memory access" in r.stderr:
        pytest.exit("iter_driver faulted (%d): nothing more is started on this device\n%s" % (r.returncode, r.stderr),
                    returncode=3)
    assert r.returncode == 0, r.stderr
    cur = _Cursor(open(o, "rb").read())
    got = []
    for c, e in zip(cmds, exp):
        g = parse_one(cur, c)
        if c[0] == "open":
            got.append(g)
            continue
        try:
            compare_one(c, g, e)
        except AssertionError:
            _keep(data, _short(c[:4] if c[0] != "scan_batch" else c[:2]))
            raise
        got.append({k: v for k, v in g.items() if k not in ("records", "queries")})
    assert cur.p == len(cur.d)
    return got, exp


def _scans(k, shapes=5):
    """the scan shapes of test_seek_gpu._bulk_check (5), or of the irregular-index test (3)"""
    if shapes == 5:
        sh = (("from", k, b""), ("prefix", k[:3], b""), ("prefix", k, b""), ("range", k, k + b"\xff"),
              ("range", k[:2], k))
    else:
        sh = (("from", k, b""), ("prefix", k[:2], b""), ("range", k, k + b"\xff"))
    return [("scan", m, k1, k2, 1 << 62) for m, k1, k2 in sh]


# ---------------------------------------------------------------- the cases (built without a GPU)
WELL_FORMED = [(1024, 4, 0), (256, 1, 0), (4096, 16, 0), (1024, 4, 1), (2048, 3, 2), (1024, 4, 5)]


@functools.lru_cache(maxsize=None)
def well_formed_case(bs, iv, comp, v1=False):
    rng = np.random.default_rng(bs + iv + comp)
    recs = corpus.random_records(rng, 4000, 0, 30, 0, 120)
    data, _ = ts._write(recs, bs, iv, comp)
    if v1:
        data = corpus.to_v1(data)
    cmds = []
    for verify in (True, False):
        cmds.append(("open", verify))
        for k in ts._probe_keys(rng, recs, 24):
            cmds += _scans(k) + [("get", k)]
        cmds.append(("len",))
    return bytes(data), cmds


def _quirk_case():
    recs = [(b"k%05d" % i, b"v%d" % i) for i in range(3000)]
    data, _ = ts._write(recs, 512, 4)
    cmds = [("open", True),
            ("iter", "from", b"k01000", b"", [3, ("seek", b"k00002"), 2, ("seek", b"k02999"), 5, ("seek", b"zzz"), 3,
                                              ("seek", b"k00500"), 4]),
            ("iter", "iter", b"", b"", [10, ("seek", b"k00003"), 3, 400, ("seek", b"k01500"), 2]),
            ("iter", "range", b"k00100", b"k00400", [20, ("seek", b"k00390"), 50]),
            ("open", False),
            ("iter", "prefix", b"k001", b"", [50, ("seek", b"k0019"), 30, 200])]
    return bytes(data), cmds


def _kat():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "kat.json")))["seek_kat"]


def _kat_case():
    kat = _kat()
    recs = [(k.encode(), bytes([0x41 + i]) * kat["value_len"]) for i, k in enumerate(kat["keys"])]
    data, _ = ts._write(recs, kat["block_size"], kat["restart_interval"])
    cmds = [("open", True)]
    for sc in kat["scripts"]:
        ops = [o if isinstance(o, int) else ("seek", o[1].encode()) for o in sc["ops"]]
        cmds.append(("iter", sc["mode"], sc["key"].encode(), b"", ops))
    return bytes(data), cmds


def _random_scripts(rng, recs, n, nops, nexts, pseek, modes=("iter", "from", "prefix", "range")):
    cmds = []
    for _ in range(n):
        keys = ts._probe_keys(rng, recs, 8)
        ops = []
        for _ in range(int(rng.integers(*nops))):
            if rng.random() < pseek:
                ops.append(("seek", keys[int(rng.integers(0, len(keys)))]))
            else:
                ops.append(int(rng.choice(nexts)))
        mode = str(rng.choice(list(modes)))
        k = keys[int(rng.integers(0, len(keys)))]
        cmds.append(("iter", mode, k if mode != "prefix" else k[:2], k + b"\x80", ops))
    return cmds


@functools.lru_cache(maxsize=None)
def stateful_case(name):
    """test_stateful_random_scripts: "plain", "zlib", and "corrupt" (restart entries with shared != 0)"""
    comp = 2 if name == "zlib" else 0
    rng = np.random.default_rng(90 + comp)
    recs = corpus.random_records(rng, 2500, 0, 24, 0, 90)
    data, (off, ln) = ts._write(recs, 700, 3, comp)
    files = [(bytes(data), True)]
    if comp == 0:
        files.append((ts._corrupt_restart_shared(data, off, ln, rng, 10), False))
    out = []
    for d, verify in files:
        out.append((d, [("open", verify)] + _random_scripts(rng, recs, 12, (2, 9), [1, 2, 7, 40, 300], 0.45)))
    return out[1 if name == "corrupt" else 0]


@functools.lru_cache(maxsize=None)
def kcap_case():
    """the key capacity a re-seeked BlockIter keeps (src/reader.rs:327-329, src/block.rs:106-112, :132):
    one entry in the last restart interval of block 0 gets a `shared` that a fresh iterator's key Vec
    cannot hold at that point and the held iterator's can.  into_iter() holds block 0 (offset 0 =
    block_offset); next() up to that interval grows the capacity; seek(a key of block 0) re-seeks the
    held block to its separator with that capacity and passes the entry; a fresh iter_from(separator)
    panics on it.  The first (file seed, entry, shared) for which the oracle says so is taken."""
    import pyoracle
    for seed in range(90, 110):
        rng = np.random.default_rng(seed)
        recs = corpus.random_records(rng, 300, 0, 24, 0, 90)
        data, (off, ln) = ts._write(recs, 1024, 3)
        keys = [k for k, _ in recs]
        sep = pyoracle.index_records(bytes(data))[0][0]
        o, L = int(off[0]), int(ln[0])
        nr = int.from_bytes(data[o + L - 4: o + L], "little")
        ro = L - 4 * (nr + 1)
        last = int.from_bytes(data[o + ro + 4 * (nr - 1): o + ro + 4 * nr], "little")
        walked = 3 * (nr - 1) - 1                                 # next() calls that stay before the last interval
        p = last + 3 + data[o + last + 1] + data[o + last + 2]    # the entry after the last restart entry
        if p + 3 > ro:
            continue
        for sh in range(9, 64):
            d = bytearray(data)
            d[o + p] = sh
            d = bytes(d)
            ops = [walked, ("seek", keys[1]), 5]
            live = pyoracle.iter_script(d, "iter", b"", b"", ops, verify=False)
            fresh = pyoracle.file_scan(d, "from", sep, verify=False)
            if fresh["end"] == END_PANIC and not fresh["records"] and live["end"] == END_NONE and \
                    live["ops"] == [(walked, 0), (0, 0), (5, 0)]:
                return d, [("open", False), ("iter", "iter", b"", b"", ops), ("scan", "from", sep, b"", 1 << 62)]
    raise AssertionError("no entry found whose outcome depends on the held key capacity")


@functools.lru_cache(maxsize=None)
def restart_shared_case(seed):
    rng = np.random.default_rng(40 + seed)
    recs = corpus.random_records(rng, 3000, 1, 24, 0, 60)
    data, (off, ln) = ts._write(recs, 1024, 4)
    bad = ts._corrupt_restart_shared(data, off, ln, rng, 12)
    assert bad != data
    cmds = [("open", False)]
    for k in ts._probe_keys(rng, recs):
        cmds += _scans(k)
    return bad, cmds


# test_bulk_random_corruption's seed 77 flips no byte the reference minds (no panic, no Err in any
# scan); 85 is the first seed after it whose six files meet every corpus condition below
FLIP_SEED = 85


@functools.lru_cache(maxsize=None)
def _flip_cases():
    rng = np.random.default_rng(FLIP_SEED)
    recs = corpus.random_records(rng, 1500, 0, 20, 0, 40)
    data, (off, ln) = ts._write(recs, 512, 2)
    out = []
    for t in range(6):
        d = bytearray(data)
        for _ in range(4):
            b = int(rng.integers(0, off.size))
            d[int(off[b]) + int(rng.integers(0, int(ln[b])))] ^= int(rng.integers(1, 256))
        cmds = [("open", False)]
        for k in ts._probe_keys(rng, recs):
            cmds += _scans(k)
        out.append((bytes(d), cmds))
    # one flipped content byte, checksums verified: the scans that reach the block panic there
    b = 1
    d = bytearray(data)
    d[int(off[b]) + int(ln[b]) // 2] ^= 0x40
    cmds = [("open", True)]
    for k in ts._probe_keys(rng, recs):
        cmds += _scans(k)
    out.append((bytes(d), cmds))
    return out


def flip_case(t):
    return _flip_cases()[t]


@functools.lru_cache(maxsize=None)
def compressed_get_case(comp):
    """a snappy (1) / zlib (2) file with one data block whose stream no longer decompresses, read
    with verification off: Reader::get for keys in, before and after that block.  A key just past
    the last key of the block before it runs next() into the damaged block: Some(Err), and
    Reader::get returns the old block iterator's value (src/reader.rs:111-122, :376-379)"""
    import pyoracle
    rng = np.random.default_rng(5)
    recs = corpus.random_records(rng, 2000, 1, 20, 0, 50)
    data, (off, ln) = ts._write(recs, 1024, 8, comp)
    b = off.size // 2
    d = bytearray(data)
    if comp == 1:
        d[int(off[b])] ^= 0x15               # the stream's uncompressed length no longer matches
    else:
        d[int(off[b]) + int(ln[b]) // 2] ^= 0x40
    keys = [k for k, _ in recs]
    ikeys = [k for k, _ in pyoracle.index_records(bytes(data))]
    probes = []
    for j in (b - 2, b - 1, b, b + 1):
        lo = bisect.bisect_right(keys, ikeys[j - 1])          # block j holds keys (ikeys[j-1], ikeys[j]]
        hi = bisect.bisect_right(keys, ikeys[j]) - 1
        probes += [keys[lo], keys[lo][:-1], keys[(lo + hi) // 2], keys[(lo + hi) // 2] + b"\x00", keys[hi],
                   keys[hi] + b"\x00", ikeys[j]]
    cmds = [("open", False)] + [("get", k) for k in probes]
    cmds += [("scan", "from", keys[bisect.bisect_right(keys, ikeys[b - 2]) + 1], b"", 1 << 62)]
    return bytes(d), cmds, b


# test_stateful_live_index_iterator's seeds 11 / 12 / 13 miss a corpus condition each (no panic; too
# few clean ends); these are the first seeds after them that meet all of them
IRREGULAR_SEED = {"restart": 20, "shared": 14, "bytes": 47}


@functools.lru_cache(maxsize=None)
def _irregular_cases(kind):
    """test_stateful_live_index_iterator: six damaged copies, five scripts and 18 scans each"""
    rng = np.random.default_rng(IRREGULAR_SEED[kind])
    recs = corpus.random_records(rng, 3000, 1, 20, 0, 40)
    data, _ = ts._write(recs, 256, 2)
    out = []
    for t in range(6):
        bad = ts._corrupt_index(data, rng, kind)
        cmds = [("open", False)] + _random_scripts(rng, recs, 5, (3, 10), [1, 3, 20, 200], 0.5)
        for k in ts._probe_keys(rng, recs, 6):
            cmds += _scans(k, 3)
        out.append((bad, cmds))
    return out


@functools.lru_cache(maxsize=None)
def _long_key_cases():
    """test_keys_over_64kib, its scans in four parts (a scan yields megabytes: keys of up to 200 KiB)"""
    rng = np.random.default_rng(64)
    recs = ts._long_key_records(rng, 40)
    data, _ = ts._write(recs, 600_000, 2)
    data = bytes(data)
    scans = []
    for k in ts._probe_keys(rng, recs):
        scans.append(_scans(k))
    rest = [("open", True)] + [("get", k) for k in ts._probe_keys(rng, recs, 10)]
    for t in range(6):
        keys = ts._probe_keys(rng, recs, 6)
        ops = [("seek", keys[int(rng.integers(0, len(keys)))]) if rng.random() < 0.5 else int(rng.choice([1, 3, 30]))
               for _ in range(6)]
        rest.append(("iter", "from", keys[t % len(keys)], b"", ops))
    out = {"scans-%d" % i: (data, [("open", True)] + sum(scans[i::4], [])) for i in range(4)}
    out["get-scripts"] = (data, rest)
    for kind in ("restart", "shared"):
        bad = ts._corrupt_index(data, rng, kind)
        keys = ts._probe_keys(rng, recs, 6)
        ops = [("seek", keys[1]), 3, ("seek", keys[2]), 5, ("seek", keys[0]), 40]
        out["index-" + kind] = (bad, [("open", False), ("iter", "iter", b"", b"", ops)])
    return out


SCAN_BATCH_FILES = ["random-1024-4", "random-1024-4-snappy", "random-2048-3-zlib", "random-1024-4-v1"]


@functools.lru_cache(maxsize=None)
def scan_batch_case(name):
    data, recs, qs, lim = su.case(name[:-3] if name.endswith("-v1") else name)
    if name.endswith("-v1"):
        data = corpus.to_v1(data)
    qs, lim = tuple(qs), tuple(lim)
    cmds = [("open", True), ("scan_batch", 64, qs, lim, name), ("scan_batch", 4, qs, lim, name)]
    return data, cmds, recs


def _handed_back(oracle, name, max_blocks=4):
    """per query of scan_batch_case(name): True where its iteration opens more than max_blocks data blocks"""
    data, cmds, recs = scan_batch_case(name)
    keys = [k for k, _ in recs]
    v2 = su.case(name[:-3])[0] if name.endswith("-v1") else data      # the same separators, V2 framing
    ikeys = [k for k, _ in oracle.index_records(v2)]
    out = []
    for q, m in zip(cmds[1][2], cmds[1][3]):
        e = su.expected(oracle, data, q, m, True, tag=name)
        out.append(su.span(ikeys, keys, q, len(e["records"]))[2] > max_blocks)
    return out


# ---------------------------------------------------------------- GPU tests: one driver run each
def _zstd_or_skip(comp):
    if comp == 5:
        import mtblx
        if mtblx.lib().mtblx_codec_available(5) != 1:
            pytest.skip("libzstd.so.1 not on this host")


@pytest.mark.gpu
@pytest.mark.parametrize("bs,iv,comp", WELL_FORMED)
def test_well_formed_files(oracle, tmp_path, bs, iv, comp):
    """scans, get and len over 27 probe keys, checksums on and off"""
    _zstd_or_skip(comp)
    data, cmds = well_formed_case(bs, iv, comp)
    got, exp = run_case(oracle, tmp_path, data, cmds)
    assert all(g["code"] == 0 for c, g in zip(cmds, got) if c[0] in ("open", "len"))
    assert sum(len(e["records"]) > 0 for c, e in zip(cmds, exp) if c[0] == "get") >= 8


@pytest.mark.gpu
def test_well_formed_v1_file(oracle, tmp_path):
    data, cmds = well_formed_case(1024, 4, 0, True)
    got, exp = run_case(oracle, tmp_path, data, cmds)
    assert all(g["code"] == 0 for c, g in zip(cmds, got) if c[0] in ("open", "len"))
    assert exp[-1]["version"] == 0


@pytest.mark.gpu
def test_stateful_seek_quirk(oracle, tmp_path):
    """seek back into the first block after iter_from: block_offset is still 0 and block 0's offset
    is 0, so the reference re-seeks the block it holds (not block 0)"""
    data, cmds = _quirk_case()
    got, exp = run_case(oracle, tmp_path, data, cmds)
    assert exp[1]["records"][3][0] != b"k00002"          # the quirk is really exercised


@pytest.mark.gpu
def test_seek_kat(oracle, tmp_path):
    """the hand-derived ReaderIntoIter::seek vectors (tests/golden/kat.json seek_kat)"""
    data, cmds = _kat_case()
    got, exp = run_case(oracle, tmp_path, data, cmds)
    for sc, e in zip(_kat()["scripts"], exp[1:]):
        assert [k.decode() for k, _ in e["records"]] == sc["yields"], sc["why"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["plain", "zlib", "corrupt"])
def test_stateful_random_scripts(oracle, tmp_path, name):
    data, cmds = stateful_case(name)
    run_case(oracle, tmp_path, data, cmds)


@pytest.mark.gpu
def test_held_key_capacity(oracle, tmp_path):
    """a seek that re-seeks the held block hands its key capacity on (kcap_now)"""
    data, cmds = kcap_case()
    got, exp = run_case(oracle, tmp_path, data, cmds)
    assert (got[1]["code"], got[2]["code"]) == (END_NONE, END_PANIC)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2])
def test_corrupt_restart_shared(oracle, tmp_path, seed):
    data, cmds = restart_shared_case(seed)
    got, _ = run_case(oracle, tmp_path, data, cmds)
    assert got[0]["code"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("t", range(6))
def test_random_corruption(oracle, tmp_path, t):
    data, cmds = flip_case(t)
    run_case(oracle, tmp_path, data, cmds)


@pytest.mark.gpu
def test_checksum_mismatch_panics(oracle, tmp_path):
    """one flipped content byte, checksums verified: the scans that reach the block end in Panic
    after the oracle's records, the others are clean"""
    data, cmds = flip_case(6)
    got, exp = run_case(oracle, tmp_path, data, cmds)
    ends = [g["code"] for g in got[1:]]
    assert set(ends) == {END_NONE, END_PANIC}


@pytest.mark.gpu
@pytest.mark.parametrize("comp", [1, 2])
def test_compressed_get_after_error(oracle, tmp_path, comp):
    data, cmds, _ = compressed_get_case(comp)
    run_case(oracle, tmp_path, data, cmds)


@functools.lru_cache(maxsize=None)
def _seen_irregular(kind):
    """how many of the six damaged copies the device finds irregular (mtblx.reader.index_regular)"""
    from mtblx import reader as rd
    n = 0
    for bad, _ in _irregular_cases(kind):
        try:
            n += not rd.ReaderBuilder().verify_checksums(False).read(bad).index_regular()
        except (rd.MtblError, rd.ReferencePanic):
            pass
    return n


@pytest.mark.gpu
@pytest.mark.parametrize("t", range(6))
@pytest.mark.parametrize("kind", ["restart", "shared", "bytes"])
def test_irregular_index(oracle, tmp_path, kind, t):
    """the live index iterator (ix_seek / ix_next / ix_load) on a damaged index block"""
    data, cmds = _irregular_cases(kind)[t]
    run_case(oracle, tmp_path, data, cmds)
    if kind != "bytes":
        assert _seen_irregular(kind) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["scans-0", "scans-1", "scans-2", "scans-3", "get-scripts", "index-restart", "index-shared"])
def test_keys_over_64kib(oracle, tmp_path, name):
    """keys of 66-200 KiB: the key-buffer retry of the emitting seek and of the capacity replay"""
    data, cmds = _long_key_cases()[name]
    run_case(oracle, tmp_path, data, cmds)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCAN_BATCH_FILES)
def test_scan_batch(oracle, tmp_path, name):
    data, cmds, _ = scan_batch_case(name)
    got, _ = run_case(oracle, tmp_path, data, cmds)
    qs = cmds[1][2]
    if "snappy" in name or "zlib" in name:
        assert not any(got[1]["served"]) and not any(got[2]["served"])
        return
    scans = [i for i, q in enumerate(qs) if q[0] in ("prefix", "range")]
    for g, max_blocks in ((got[1], 64), (got[2], 4)):
        back = _handed_back(oracle, name, max_blocks)
        for i, q in enumerate(qs):
            if q[0] != "from":
                assert (g["served"][i] == 0) == back[i], (max_blocks, q, g["served"][i])
    n = sum(got[2]["served"][i] == 0 for i in scans)
    assert 0.01 * len(scans) <= n <= 0.4 * len(scans), (n, len(scans))


# ---------------------------------------------------------------- no GPU: the driver, the corpus
def test_iter_driver_is_built():
    """the `cpp` target of the Makefile builds the driver against libmtblx.so"""
    assert os.path.exists(EXE), "build/iter_driver not built (make -C oxidized-mtbl_amd cpp)"
    out = subprocess.run(["nm", "-D", "--undefined-only", EXE], capture_output=True, text=True).stdout
    assert "mtblx_block_seek_batch" in out.split() and "mtblx_scan_plan" in out.split()


def test_script_encoding_round_trip():
    """encode() and parse_one() agree with the layout iter_driver.cpp documents"""
    cmds = [("open", False), ("iter", "range", b"a\0", b"\xff", [3, ("seek", b"")]), ("get", b"k"), ("len",),
            ("scan", "prefix", b"p", b"", 7), ("scan_batch", 4, (("range", b"a", b"b"), ("from", b"c")), (None, 0), None)]
    assert encode(cmds) == (b"O\0" b"I\3" + _b(b"a\0") + _b(b"\xff") + b"\2\0\0\0" b"\0\3\0\0\0\0\0\0\0" b"\1" + _b(b"") +
                            b"G" + _b(b"k") + b"L" b"S\2" + _b(b"p") + _b(b"") + b"\7\0\0\0\0\0\0\0" +
                            b"B\4\0\0\0\2\0\0\0" b"\3" + _b(b"a") + _b(b"b") + b"\0" + bytes(8) +
                            b"\0" + _b(b"c") + _b(b"") + b"\1" + bytes(8))
    out = (b"O\1" + _b(b"InvalidBlock") + b"I\3" + _b(b"Io") + b"\1\0\0\0" + struct.pack("<QB", 2, 2) +
           struct.pack("<Q", 1) + _b(b"k") + _b(b"") + b"G\0" + _b(b"") + _b(b"val") + b"L\0" + _b(b"") +
           struct.pack("<Q", 9))
    cur = _Cursor(out)
    assert parse_one(cur, cmds[0]) == dict(code=1, err="InvalidBlock")
    assert parse_one(cur, cmds[1]) == dict(code=3, err="Io", ops=[(2, 2)], records=[(b"k", b"")])
    assert parse_one(cur, cmds[2]) == dict(code=0, err="", value=b"val")
    assert parse_one(cur, cmds[3]) == dict(code=0, err="", len=9) and cur.p == len(out)


def _stats(oracle, cases):
    """over the scripts and scans of some cases: (n, ended at open or before the first record,
    ended in PANIC / LOOP, Err during next, ended cleanly after more than 10 records)"""
    n = early = panic = err_next = clean = 0
    for data, cmds in cases:
        for c, e in zip(cmds, expect_all(oracle, data, cmds)):
            if c[0] not in ("iter", "scan"):
                continue
            n += 1
            early += e["end"] != END_NONE and not e["records"]
            panic += e["end"] in (END_PANIC, END_LOOP)
            err_next += e["end"] == END_ERR_NEXT or any(code == 2 for _, code in e.get("ops", ()))
            clean += e["end"] == END_NONE and len(e["records"]) > 10
    return n, early, panic, err_next, clean


def _groups():
    """the corrupt-data cases taken together (restart entries with shared != 0 only ever take
    BlockIter::seek's early return, src/block.rs:167-170: no seed makes such a file panic or err, so
    it cannot meet the conditions alone), and the six damaged copies of each index damage kind"""
    g = {"corrupt-data": lambda: [restart_shared_case(1), restart_shared_case(2), stateful_case("corrupt")] +
         list(_flip_cases())}
    for kind in IRREGULAR_SEED:
        g["index-" + kind] = functools.partial(_irregular_cases, kind)
    return g


_group_stats = {}


def _group_stat(oracle, name):
    if name not in _group_stats:
        _group_stats[name] = [_stats(oracle, [c]) for c in _groups()[name]()]
    return _group_stats[name]


@pytest.mark.parametrize("name", list(_groups()))
def test_corpus_conditions(oracle, name):
    """what keeps the corrupt and irregular cases from passing vacuously, by the oracle alone: at
    most half of the scripts and scans end at open or before their first record (in every file, too),
    one at least ends in a panic or never returns, a third at least end cleanly after more than 10
    records; and an Err during next() occurs among the corrupt-data cases"""
    per_case = _group_stat(oracle, name)
    n, early, panic, err_next, clean = (sum(x) for x in zip(*per_case))
    print(name, dict(n=n, early=early, panic=panic, err_next=err_next, clean=clean))
    assert all(2 * c[1] <= c[0] for c in per_case), per_case
    assert 2 * early <= n, (early, n)
    assert panic >= 1
    assert 3 * clean >= n, (clean, n)
    if name == "corrupt-data":
        assert err_next >= 1


def _index_irregular(data):
    """mtblx_entry_offsets' rule on the host, for index entries with one-byte varints: a restart
    entry with shared != 0, an entry with shared past the previous key's length, or an interval
    whose chain misses the next restart point"""
    o, L = ts._index_window(data)
    nr = int.from_bytes(data[o + L - 4: o + L], "little")
    ro = L - 4 * (nr + 1)
    rps = [int.from_bytes(data[o + ro + 4 * i: o + ro + 4 * i + 4], "little") for i in range(nr)]
    p, klen = rps[0], 0
    while p + 3 <= ro:
        sh, ns, vl = data[o + p], data[o + p + 1], data[o + p + 2]
        if max(sh, ns, vl) >= 128 or (p in rps and sh) or sh > klen:
            return True
        klen = sh + ns
        nxt = p + 3 + ns + vl
        if any(p < r < nxt for r in rps):
            return True
        p = nxt
    return p != ro


@pytest.mark.parametrize("kind", ["restart", "shared"])
def test_index_damage_is_irregular(kind):
    """at least one of the six damaged copies has an irregular index (the GPU test asserts it with
    mtblx.reader's index_regular() on the same bytes)"""
    assert sum(_index_irregular(bad) for bad, _ in _irregular_cases(kind)) >= 1
    assert not _index_irregular(well_formed_case(1024, 4, 0)[0])


def test_held_key_capacity_corpus(oracle):
    """kcap_case() finds its entry: the script ends cleanly with the records after its last seek,
    the fresh scan of the same block panics before its first record"""
    data, cmds = kcap_case()
    exp = expect_all(oracle, data, cmds)
    assert exp[1]["end"] == END_NONE and exp[1]["ops"][2] == (5, 0)
    assert exp[2]["end"] == END_PANIC and not exp[2]["records"]


@pytest.mark.parametrize("comp", [1, 2])
def test_compressed_get_corpus(oracle, comp):
    """the damaged block is an Err(Io) of the decompressor; some get returns the held value of the
    block before it, some get errs at construction, and the others find their keys or nothing"""
    data, cmds, b = compressed_get_case(comp)
    exp = expect_all(oracle, data, cmds)
    assert (exp[-1]["end"], exp[-1]["err"]) == (END_ERR_NEXT, "Io") and len(exp[-1]["records"]) > 3
    gets = [(c[1], e) for c, e in zip(cmds, exp) if c[0] == "get"]
    held = [k for k, e in gets if e["end"] == END_NONE and e["records"] and e["records"][0][0] != k]
    assert held                                               # Reader::get after Some(Err)
    assert sum(e["end"] == END_ERR_OPEN and e["err"] == "Io" for _, e in gets) >= 3
    assert sum(e["end"] == END_NONE and bool(e["records"]) and e["records"][0][0] == k for k, e in gets) >= 8
    assert sum(e["end"] == END_NONE and not e["records"] for _, e in gets) >= 3


@pytest.mark.parametrize("name", SCAN_BATCH_FILES)
def test_scan_batch_corpus(oracle, name):
    """between 1 and 40 % of the prefix / range queries open more than 4 data blocks"""
    qs = scan_batch_case(name)[1][1][2]
    back = _handed_back(oracle, name)
    scans = [i for i, q in enumerate(qs) if q[0] in ("prefix", "range")]
    n = sum(back[i] for i in scans)
    assert len(scans) >= 150 and 0.01 * len(scans) <= n <= 0.4 * len(scans), (n, len(scans))


def test_quirk_and_kat_corpus(oracle):
    data, cmds = _quirk_case()
    assert oracle.iter_script(data, *cmds[1][1:], verify=True)["records"][3][0] != b"k00002"
    data, cmds = _kat_case()
    assert data == oracle.write_file([(k.encode(), bytes([0x41 + i]) * _kat()["value_len"])
                                      for i, k in enumerate(_kat()["keys"])], _kat()["block_size"],
                                     _kat()["restart_interval"])
    for sc, c in zip(_kat()["scripts"], cmds[1:]):
        assert [k.decode() for k, _ in oracle.iter_script(data, *c[1:], verify=True)["records"]] == sc["yields"]
