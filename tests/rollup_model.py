"""The host definition of a rollup (include/mtblx.h "Rollups"), written from its text with
Reduce.fold and Reduce.encode.  Pure Python: no torch, no library call.

A group rule is ("length", L) or ("delimiter", byte, count); `as_rule` takes a mtblx GroupBy too."""
import bisect


def as_rule(group):
    if isinstance(group, tuple):
        return group
    if group.kind == "length":
        return ("length", group.length_)
    return ("delimiter", group.delim, group.count)


def gkey(key: bytes, group) -> bytes:
    rule = as_rule(group)
    if rule[0] == "length":
        L = rule[1]
        assert L >= 1
        return key[:L] if len(key) > L else key
    _, byte, count = rule
    assert 0 <= byte <= 255 and count >= 1
    seen = 0
    for i, b in enumerate(key):
        if b == byte:
            seen += 1
            if seen == count:
                return key[: i + 1]
    return key


def heads(records, group, seg_off=None):
    """the head flag of every record"""
    n = len(records)
    seg_off = [0, n] if seg_off is None else list(seg_off)
    assert seg_off[0] == 0 and seg_off[-1] == n and all(a <= b for a, b in zip(seg_off, seg_off[1:]))
    starts = set(seg_off[:-1])
    out = []
    for r, (k, _) in enumerate(records):
        out.append(r == 0 or r in starts or gkey(k, group) != gkey(records[r - 1][0], group))
    return out


def rollup(records, group, reduce, seg_off=None):
    """-> dict: keys, values (per group), fields (tuples of unsigned ints), nrec, nbad, grp_rec
    ([G + 1]), seg_grp ([nseg + 1])"""
    n = len(records)
    seg_off = [0, n] if seg_off is None else list(seg_off)
    hd = heads(records, group, seg_off)
    grp_rec = [r for r in range(n) if hd[r]] + [n]
    G = len(grp_rec) - 1
    out = dict(keys=[], values=[], fields=[], nrec=[], nbad=[], grp_rec=grp_rec, seg_grp=[])
    for g in range(G):
        a, b = grp_rec[g], grp_rec[g + 1]
        f, nrec, nbad = reduce.fold([v for _, v in records[a:b]])
        out["keys"].append(gkey(records[a][0], group))
        out["values"].append(reduce.encode(f))
        out["fields"].append(tuple(f))
        out["nrec"].append(nrec)
        out["nbad"].append(nbad)
    for off in seg_off:
        out["seg_grp"].append(bisect.bisect_left(grp_rec, off, 0, G))   # the groups that begin before record `off`
    return out


def groups_of(model, q):
    """segment q's groups as Rollup.groups(q) gives them: [(key, fields, nrec, nbad)]"""
    a, b = model["seg_grp"][q], model["seg_grp"][q + 1]
    return [(model["keys"][g], model["fields"][g], model["nrec"][g], model["nbad"][g]) for g in range(a, b)]
