"""Set operations on the device Merger (mtblx.Select over mtblx_merge_plan_select /
mtblx_merge_seg_plan_select, csrc/merge_dev.h k_group_select) against tests/select_model.py: the
keys, and the values of every mode.

The model is the definition (include/mtblx.h "Set operations") on top of merger_model.multi_iter;
the values of a kept group are compared in source order, this library's promise."""
import ctypes as C
import functools

import numpy as np
import pytest

import merger_model as mm
import merger_scan_util as U
import rollup_model
import select_model as sm

pytestmark = pytest.mark.gpu

KTILE, KEMIT = 1024, 256   # csrc/merge_dev.h kTile, kEmitTile


def _mods():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mtblx import _lib, encode, merger, reader
    return torch, _lib, encode, merger, reader


def _rules(nsrc):
    from mtblx import Select
    return {"union": Select.union(), "intersection": Select.intersection(nsrc),
            "difference": Select.difference(0, range(1, nsrc)), "exactly_one": Select.exactly_one(),
            "at_least_2": Select.at_least(2)}


def _reds():
    from mtblx import Reduce
    return Reduce("sum", "min", "max"), Reduce("sum", "min", "max", encoding="varint")


def _fields(rng):
    return [int(rng.integers(0, 1 << 62)), int(rng.integers(0, 1 << 20)), int(rng.integers(0, 300))]


def _two_codings(lists):
    """lists of (key, fields) -> the same sources with u64le values and with varint values"""
    u64, var = _reds()
    return ([[(k, u64.encode(f)) for k, f in r] for r in lists], [[(k, var.encode(f)) for k, f in r] for r in lists])


def _dev(lists):
    encode = _mods()[2]
    return [encode.DeviceRecords.from_list(r) for r in lists]


def _check_modes(lists_u64, lists_var, sel, dev_u64=None, dev_var=None):
    """"groups", "concat", "first", "last" and both Reduce encodings of merge_records with `sel`"""
    torch, _lib, encode, merger, reader = _mods()
    u64, var = _reds()
    dev_u64 = dev_u64 or _dev(lists_u64)
    dev_var = dev_var or _dev(lists_var)
    want = sm.select_groups(lists_u64, sel)
    assert merger.merge_records(dev_u64, "groups", select=sel).to_list() == want
    for mode in ("concat", "first", "last"):
        got = merger._records_list(merger.merge_records(dev_u64, mode, select=sel))
        assert got == U.merged(want, U.PICK[mode]), mode
    got = merger._records_list(merger.merge_records(dev_u64, u64, select=sel))
    assert got == sm.select_merge(lists_u64, sel, u64.host)
    got = merger._records_list(merger.merge_records(dev_var, var, select=sel))
    assert got == sm.select_merge(lists_var, sel, var.host)
    return want


# ---------------------------------------------------------------- the small sweep
@functools.lru_cache(maxsize=None)
def _sweep_sources(nsrc):
    rng = np.random.default_rng(4200 + nsrc)
    pool = sorted({bytes(rng.choice([0x61, 0x62, 0x00, 0xFF], size=int(rng.integers(1, 12))).tolist())
                   for _ in range(160)})
    lists = []
    for s in range(nsrc):
        p = (0.9, 0.5, 0.2)[s % 3]
        lists.append([(k, _fields(rng)) for k in pool if rng.random() < p or k == pool[7]])
    lists[0].append((b"zz-only-first", _fields(rng)))        # the keys one source alone holds
    lists[-1].append((b"zz-only-last", _fields(rng)))
    return _two_codings([sorted(r) for r in lists])


@pytest.mark.parametrize("nsrc", [1, 2, 3, 8, 64])
def test_small_sweep(oracle, nsrc):
    torch, _lib, encode, merger, reader = _mods()
    lists_u64, lists_var = _sweep_sources(nsrc)
    dev_u64, dev_var = _dev(lists_u64), _dev(lists_var)
    readers = [reader.Reader(mm.make_source(r)) for r in lists_u64]
    sizes = {}
    for name, sel in _rules(nsrc).items():
        want = _check_modes(lists_u64, lists_var, sel, dev_u64, dev_var)
        sizes[name] = len(want)
        # a callable merge function runs over the selected groups of two or more, on the host
        calls = []

        def cat(key, values):
            calls.append((key, len(values)))
            return b"|".join(values)

        m = merger.Merger.builder(cat).extend(readers).select(sel).build()
        assert list(m.into_merge_iter()) == sm.select_merge(lists_u64, sel, lambda k, vs: b"|".join(vs)), name
        assert calls == [(k, len(vs)) for k, vs in want if len(vs) > 1]
        assert list(m.into_iter()) == want
    n = len(sm.select_groups(lists_u64, None))
    assert sizes["union"] == n and sizes["intersection"] >= 1          # pool[7] lies in every source
    assert sizes["exactly_one"] + sizes["at_least_2"] == n
    if nsrc > 1:
        assert 0 < sizes["difference"] < sizes["exactly_one"] < n and 0 < sizes["at_least_2"] < n
    else:
        assert sizes["at_least_2"] == 0 and sizes["exactly_one"] == sizes["difference"] == n


# ---------------------------------------------------------------- tile edges
def _layout(keys):
    """[(key, sources holding it)] -> (lists of (key, fields), the merged position where every key's group starts)"""
    rng = np.random.default_rng(77)
    lists = [[] for _ in range(64)]
    starts, pos = [], 0
    for k, srcs in keys:
        starts.append(pos)
        pos += len(srcs)
        for s in srcs:
            lists[s].append((k, _fields(rng)))
    return lists, starts + [pos]


@functools.lru_cache(maxsize=None)
def _edge_layout_a():
    """64 sources share 41 keys; source 63 holds every other one, so groups of 64 and 63 alternate and
    a rule on source 63 rejects alternate groups.  A first key in 30 sources shifts the groups off the
    multiples of 64: one straddles record 256 (kEmitTile), one 1024 (kTile), one 2048."""
    keys = [(b"a-front", tuple(range(30)))]
    keys += [(b"k%03d" % i, tuple(range(64 if i % 2 == 0 else 63))) for i in range(41)]
    return keys


@functools.lru_cache(maxsize=None)
def _edge_layout_b():
    """a kept group of ONE is the last group of tile 0 that ends inside it, and the rejected group of
    64 after it crosses record 1024: the records of tile 1 before its first kept head are flagged
    out without the head bit (the reducers' edge logic must not take them for the group's tail)."""
    keys = [(b"f%03d" % i, tuple(range(63))) for i in range(15)]      # 945 records
    keys += [(b"g-55", tuple(range(55)))]                             # 1000
    keys += [(b"h-single", (0,))]                                     # record 1000, alone in source 0
    keys += [(b"i-all", tuple(range(64)))]                            # records 1001 .. 1064: rejected, crosses 1024
    keys += [(b"j%03d" % i, tuple(range(63 if i % 2 else 64))) for i in range(25)]   # past 2048
    return keys


def _straddlers(keys, starts, edges):
    """edge -> the index of the key whose group has records on both sides of it"""
    out = {}
    for e in edges:
        for i in range(len(keys)):
            if starts[i] < e < starts[i + 1]:
                out[e] = i
    return out


@pytest.mark.parametrize("layout", ["a", "b"])
def test_tile_edges(oracle, layout):
    from mtblx import Select
    keys = _edge_layout_a() if layout == "a" else _edge_layout_b()
    lists, starts = _layout(keys)
    lists_u64, lists_var = _two_codings(lists)
    assert 2500 < starts[-1] < 2800
    cross = _straddlers(keys, starts, (KEMIT, KTILE, 2 * KTILE))
    assert set(cross) == {KEMIT, KTILE, 2 * KTILE}, cross
    without, with63 = Select(exclude=[63]), Select(require=[63])
    if layout == "a":
        # under one of the two rules every crossing group is kept between two rejected ones, under the other the reverse
        for e, i in cross.items():
            held = [63 in keys[j][1] for j in (i - 1, i, i + 1)]
            assert held in ([True, False, True], [False, True, False]), (e, held)
    else:
        i = cross[KTILE]
        assert keys[i][0] == b"i-all" and keys[i - 1] == (b"h-single", (0,)) and starts[i - 1] == 1000
    dev_u64, dev_var = _dev(lists_u64), _dev(lists_var)
    for sel in (without, with63, Select.union(), Select(max_count=63, min_count=2)):
        assert _check_modes(lists_u64, lists_var, sel, dev_u64, dev_var)
    kept = [k for k, _ in sm.select_groups(lists_u64, without)]
    assert kept == [k for k, srcs in keys if 63 not in srcs] and 0 < len(kept) < len(keys)


# ---------------------------------------------------------------- the bare C ABI: totals, degenerate outcomes
class _Raw:
    """mtblx_merge_plan (sel is False) or mtblx_merge_plan_select (sel: a Select or None for NULL) and
    mtblx_merge_emit in `mode`, with outputs sized by the totals exactly"""

    def __init__(self, dev, sel, mode):
        torch, _lib, encode, merger, reader = _mods()
        L = __import__("mtblx").lib()
        arr = (_lib.Records * max(len(dev), 1))()
        for i, r in enumerate(dev):
            arr[i] = r.cstruct()
        n = sum(r.n for r in dev)
        wsb = int(L.mtblx_merge_workspace_bytes(n, len(dev)))
        ws = torch.full((wsb + 256,), 0xA5, dtype=torch.uint8, device="cuda")
        wp = (ws.data_ptr() + 255) & ~255
        tot = (C.c_uint64 * 8)(*([0xDEAD] * 8))
        if sel is False:
            rc = L.mtblx_merge_plan(arr, len(dev), tot, C.c_void_p(wp), wsb, None)
        else:
            spec = sel.cstruct() if sel is not None else None
            rc = L.mtblx_merge_plan_select(arr, len(dev), C.byref(spec) if spec is not None else None, tot,
                                           C.c_void_p(wp), wsb, None)
        assert rc == 0
        self.totals = [int(x) for x in tot]
        groups, kb, nv, vb = self.totals[:4]
        grouped = mode == _lib.MERGE_GROUPS
        size = {"keys": kb, "key_end": 8 * groups, "vals": vb, "val_end": 8 * (nv if grouped else groups),
                "grp_end": 8 * groups if grouped else 0}
        buf = {k: torch.full((max(v, 1),), 0xA5, dtype=torch.uint8, device="cuda") for k, v in size.items()}
        flags = torch.full((1,), 0x5A5A, dtype=torch.int32, device="cuda")
        out = _lib.Merged(buf["keys"].data_ptr(), size["keys"], buf["key_end"].data_ptr(), size["key_end"],
                          buf["vals"].data_ptr(), size["vals"], buf["val_end"].data_ptr(), size["val_end"],
                          buf["grp_end"].data_ptr(), size["grp_end"], flags.data_ptr())
        assert L.mtblx_merge_emit(arr, len(dev), mode, C.byref(out), C.c_void_p(wp), wsb, None) == 0
        torch.cuda.synchronize()
        self.flags = int(flags.item())
        self.out = {k: buf[k][: size[k]].cpu().numpy().tobytes() for k in size}
        if mode in (_lib.MERGE_FIRST, _lib.MERGE_LAST):    # vals is an upper bound there
            self.out["vals"] = self.out["vals"][: int(np.frombuffer(self.out["val_end"], np.uint64)[-1]) if groups else 0]


def test_rejects_nothing_is_the_plain_plan(oracle):
    """a rule that keeps every group: the bytes and totals[0..5] of mtblx_merge_plan + mtblx_merge_emit"""
    torch, _lib, encode, merger, reader = _mods()
    from mtblx import Select
    lists_u64, _ = _sweep_sources(8)
    lists_u64 = [[(b"", b"quirk-%d" % s)] + r if s in (2, 5) else r for s, r in enumerate(lists_u64)]
    dev = _dev(lists_u64)
    nrec = sum(len(r) for r in lists_u64)
    for mode in range(4):
        plain = _Raw(dev, False, mode)
        assert plain.totals[6:] == [0xDEAD, 0xDEAD]                   # the plain plan writes 6 words
        assert plain.totals[4] == 2 and plain.totals[2] == nrec - 2 and plain.flags == 0
        for sel in (Select.union(), Select(min_count=0, max_count=8), None):
            r = _Raw(dev, sel, mode)
            assert r.totals[:6] == plain.totals[:6] and r.totals[6:] == [0, 0] and r.flags == 0
            assert r.out == plain.out, (mode, sel)


def test_rejects_everything(oracle):
    torch, _lib, encode, merger, reader = _mods()
    from mtblx import Select
    lists_u64, lists_var = _sweep_sources(3)
    lists_u64 = [[(b"", b"q")] + r if s == 1 else r for s, r in enumerate(lists_u64)]
    dev = _dev(lists_u64)
    sel = Select(min_count=4)
    groups = sm.masked_groups(lists_u64)
    assert sm.left_out(lists_u64, sel) == (len(groups), sum(len(vs) for _, _, vs in groups))
    for mode in range(4):
        r = _Raw(dev, sel, mode)
        assert r.totals[:4] == [0, 0, 0, 0] and r.totals[5] == 0 and r.flags == 0
        assert r.totals[4] == 1                                        # the quirk's drop alone
        assert r.totals[6:] == list(sm.left_out(lists_u64, sel))
        assert all(v == b"" for v in r.out.values())
    assert merger.merge_records(dev, "groups", select=sel).to_list() == []
    u64, var = _reds()
    assert merger.merge_records(dev, u64, select=sel).n == 0
    assert merger.merge_records(_dev(lists_var), var, select=sel).n == 0
    # a partial rule: [6] and [7] count what the model leaves out, [0] and [2] what it keeps
    for sel in (Select.exactly_one(), Select.difference(0, [1, 2]), Select.at_least(2)):
        r = _Raw(dev, sel, 0)
        want = sm.select_groups(lists_u64, sel)
        assert r.totals[0] == len(want) and r.totals[2] == sum(len(vs) for _, vs in want)
        assert r.totals[6:] == list(sm.left_out(lists_u64, sel)) and r.totals[4] == 1


def test_only_empty_keys(oracle):
    """the one surviving item has the mask of the highest-numbered source"""
    torch, _lib, encode, merger, reader = _mods()
    from mtblx import Select
    lists = [[(b"", b"x0")], [(b"", b"x1")], [(b"", b"x2")]]
    dev = _dev(lists)
    for sel, want in ((Select.difference(2, [0, 1]), [(b"", [b"x2"])]), (Select.exactly_one(), [(b"", [b"x2"])]),
                      (Select(require=[0]), []), (Select.intersection(3), []), (Select.at_least(2), [])):
        assert sm.select_groups(lists, sel) == want
        assert merger.merge_records(dev, "groups", select=sel).to_list() == want
        r = _Raw(dev, sel, 0)
        assert r.totals[4] == 2 and r.totals[6:] == ([0, 0] if want else [1, 1])


# ---------------------------------------------------------------- segmented: the batched reads of a selected view
@functools.lru_cache(maxsize=None)
def _seg_case():
    rng = np.random.default_rng(31)
    pool = sorted({b"%c%c%02d" % (97 + int(rng.integers(0, 6)), 97 + int(rng.integers(0, 6)), int(rng.integers(0, 40)))
                   for _ in range(700)})
    red = _reds()[0]
    lists = []
    for s in range(3):
        keep = [k for k in pool if rng.random() < (0.7, 0.5, 0.6)[s]]
        lists.append([(b"", red.encode([s, s, s]))] + [(k, red.encode(_fields(rng))) for k in keep])
    qs = [("get", b""), ("prefix", b"")]                # only empty keys; everything (handed back under max_blocks=1)
    for i in range(66):
        k = pool[int(rng.integers(0, len(pool)))]
        k2 = pool[int(rng.integers(0, len(pool)))]
        qs += [("get", k if i % 3 else k + b"x"), ("prefix", k[: 2 + i % 2]), ("range", min(k, k2), max(k, k2))]
    return [mm.make_source(r, 1024, 4) for r in lists], lists, qs


def _seg_expect(oracle, datas, qs, sel):
    return [sm.select_groups(U.per_source(oracle, datas, q, "select-seg"), sel) for q in qs]


@pytest.mark.parametrize("rule", ["union", "intersection", "difference", "exactly_one", "at_least_2"])
def test_segmented(oracle, rule):
    torch, _lib, encode, merger, reader = _mods()
    from mtblx import GroupBy
    datas, lists, qs = _seg_case()
    assert len(qs) == 200
    sel = _rules(3)[rule]
    exp = _seg_expect(oracle, datas, qs, sel)
    assert exp[0] == ([(b"", [lists[2][0][1]])] if rule in ("union", "exactly_one") else [])   # mask 0b100
    assert any(exp) and (rule == "union" or exp != _seg_expect(oracle, datas, qs, None))
    readers = [reader.Reader(d) for d in datas]
    red = _reds()[0]
    for max_blocks in (64, 1):
        m = merger.Merger(readers, "concat", select=sel)
        res = m.scan_batch_groups(qs, max_blocks=max_blocks)
        back = [q for q in range(len(qs)) if not res.served_by_kernel(q)]
        assert (1 in back and any(qs[q][0] != "get" for q in range(len(qs)) if q not in back)) if max_blocks == 1 \
            else not back
        for q in range(len(qs)):
            assert res.groups(q) == exp[q], (q, qs[q])
            assert int(res.count[q]) == len(exp[q])
        # seg_end counts kept groups: the kernel's own segments, handed-back ones included as the kernel saw them
        off = res.grp_off.cpu().tolist()
        assert [off[q + 1] - off[q] for q in range(len(qs)) if q not in back] == [len(exp[q]) for q in range(len(qs))
                                                                                  if q not in back]
        for mode in ("first", "last"):
            rs = merger.Merger(readers, mode, select=sel).scan_batch(qs, max_blocks=max_blocks)
            assert [rs.records(q) for q in range(len(qs))] == [U.merged(e, U.PICK[mode]) for e in exp], mode
    # get_batch, reduce_batch and rollup_batch over the selected view, the Merger's Reduce joining each key's values
    m = merger.Merger(readers, red, select=sel)
    merged = [U.merged(e, lambda vs: red.host(b"", vs)) for e in exp]
    gets = [q for q in range(len(qs)) if qs[q][0] == "get"]
    gb = m.get_batch([qs[q][1] for q in gets])
    assert [gb.records(i) for i in range(len(gets))] == [merged[q] for q in gets]
    rb = m.reduce_batch(qs, max_blocks=1)
    for q in range(len(qs)):
        f, nrec, nbad = red.fold([v for _, v in merged[q]])
        assert (rb.values(q),) + tuple(rb.counts(q)) == (f, nrec, nbad), q
    ro = m.rollup_batch(qs, GroupBy.length(2), max_blocks=1)
    for q in range(len(qs)):
        assert ro.groups(q) == rollup_model.groups_of(rollup_model.rollup(merged[q], ("length", 2), red), 0), q


# ---------------------------------------------------------------- the Writer
@pytest.mark.parametrize("compression", ["None_", "Snappy"])
def test_written_files(oracle, compression):
    """diff_files and Merger(select=intersection).write_file() against the oracle Writer's file of the
    model's records.  Compressed bytes are not pinned to any compressor (the oracle's Snappy blocks
    differ from the device compressor's byte for byte, tests/test_snappy_comp_gpu.py), so with Snappy
    the file is compared where it is pinned: the records the oracle reads from it, the device
    Writer's own file of the model's records byte for byte, and the footer's compression word."""
    torch, _lib, encode, merger, reader = _mods()
    import mtblx
    from mtblx import Select, setops
    comp = getattr(mtblx.CompressionType, compression)
    rng = np.random.default_rng(5)
    pool = [b"host-%05d" % i for i in range(1500)]
    old = [(k, b"old " * int(rng.integers(1, 6))) for k in pool if rng.random() < 0.8]
    new = [(k, b"new " * int(rng.integers(1, 6))) for k in pool if rng.random() < 0.8]
    third = [(k, b"3") for k in pool if rng.random() < 0.9]
    fo, fn, f3 = (mm.make_source(r, 1024) for r in (old, new, third))
    okeys = {k for k, _ in old}
    want = sm.select_merge([new, old], Select.difference(0, [1]), lambda k, vs: vs[0])
    assert want == [(k, v) for k, v in new if k not in okeys] and 100 < len(want) < len(new)
    inter = sm.select_merge([old, new, third], Select.intersection(3), lambda k, vs: b"".join(vs))
    assert 300 < len(inter) < len(old)

    def same(got, records):
        got = got.cpu().numpy().tobytes()
        if compression == "None_":
            assert got == oracle.write_file(records, 2048, 8)
            return
        assert oracle.file_scan(got, verify=True)["records"] == records
        assert got == encode.write_file(encode.DeviceRecords.from_list(records), 2048, 8,
                                        compression=comp).cpu().numpy().tobytes()
        assert int.from_bytes(got[len(got) - 512 + 16: len(got) - 512 + 24], "little") == 1

    same(setops.diff_files(fn, fo, block_size=2048, restart_interval=8, compression=comp), want)
    same(setops.diff_files(reader.Reader(fn), reader.Reader(fo), block_size=2048, restart_interval=8,
                           compression=comp), want)
    m = merger.Merger([reader.Reader(f) for f in (fo, fn, f3)], "concat", select=Select.intersection(3))
    same(m.write_file(2048, 8, compression=comp), inter)
    if compression == "None_":
        w = mtblx.WriterBuilder().block_size(2048).block_restart_interval(8).memory()
        m.write_into(w)
        assert w.into_inner() == oracle.write_file(inter, 2048, 8)
        ro = merger.Merger([reader.Reader(f) for f in (fo, fn)], "sum_u64", select=Select.exactly_one())
        assert ro.rollup(mtblx.GroupBy.length(8), mtblx.Reduce("sum")).groups(0) == rollup_model.groups_of(
            rollup_model.rollup(sm.select_merge([old, new], Select.exactly_one(), None), ("length", 8),
                                mtblx.Reduce("sum")), 0)


# ---------------------------------------------------------------- refusals, streams
def test_refusals(oracle):
    torch, _lib, encode, merger, reader = _mods()
    from mtblx import Select
    one = encode.DeviceRecords.from_list([(b"k", b"v")])
    with pytest.raises(ValueError, match="64 sources"):
        merger.Merger([None] * 65, "concat", select=Select.union())
    with pytest.raises(ValueError, match="64 sources"):
        merger.merge_all([one] * 65, "concat", select=Select.union())
    with pytest.raises(ValueError, match="64 sources"):
        merger.merge_segments([one] * 65, [torch.tensor([0, 1], device="cuda")] * 65, "concat", select=Select.union())
    assert merger.merge_all([one] * 65, "first").n == 1              # without a selection: rounds, as ever
    with pytest.raises(ValueError, match="names source 2"):
        merger.Merger([None, None], "concat", select=Select.difference(0, [2]))
    with pytest.raises(ValueError, match="names source 2"):
        merger.merge_records([one, one], "concat", select=Select(require=[2]))
    with pytest.raises(ValueError, match="names source 1"):
        merger.MergerBuilder("concat").add(None).select(Select.intersection(2)).build()
    rd = reader.Reader(mm.make_source([(b"a", b"1"), (b"b", b"2")]))
    m = merger.Merger([rd, rd], "concat", select=Select.union())
    for kw in (dict(max_records=3), dict(max_records=[None, 0])):
        with pytest.raises(ValueError, match="max_records"):
            m.scan_batch([("from", b""), ("get", b"a")], **kw)
        with pytest.raises(ValueError, match="max_records"):
            m.scan_batch_groups([("from", b""), ("get", b"a")], **kw)
        with pytest.raises(ValueError, match="max_records"):
            m.reduce_batch([("from", b""), ("get", b"a")], "sum_u64", **kw)
    assert m.scan_batch([("from", b"")], max_records=None).records(0) == [(b"a", b"11"), (b"b", b"22")]


def test_on_a_non_default_stream(oracle):
    torch, _lib, encode, merger, reader = _mods()
    import stream_util as su
    from mtblx import Select
    lists_u64, _ = _sweep_sources(3)
    readers = [reader.Reader(mm.make_source(r)) for r in lists_u64]
    sel = Select.at_least(2)
    want = sm.select_groups(lists_u64, sel)
    qs = [("prefix", b""), ("get", want[0][0]), ("prefix", b"a")]
    exp = [sm.select_groups([[r for r in s if r[0].startswith(q[1]) and (q[0] == "prefix" or r[0] == q[1])]
                             for s in lists_u64], sel) for q in qs]

    def merged(st):
        return merger.Merger(readers, "concat", st, sel).groups()

    def written(st):   # the device Writer allocates and frees device memory itself: it waits for the whole device
        return merger.Merger(readers, "concat", st, sel).write_file(1024, 16)

    def scanned(st):
        res = merger.Merger(readers, "concat", st, sel).scan_batch_groups(qs, stream=st)
        return [res.groups(q) for q in range(len(qs))]

    file = oracle.write_file(U.merged(want, U.PICK["concat"]), 1024, 16)
    assert merged(None).to_list() == want and scanned(None) == exp    # loads the code objects outside any hold
    assert written(None).cpu().numpy().tobytes() == file
    (s,) = su.pick_streams(1)
    for config in ("current-held", "ambient"):
        assert su.run(config, merged, s).to_list() == want
        assert su.run(config, scanned, s) == exp
        assert su.host(su.run(config, written, s, device_wide=True), s).tobytes() == file
