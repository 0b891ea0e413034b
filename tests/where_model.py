"""The model of the value predicates (include/mtblx.h "Value predicates"): plain Python over record
lists, with Where.keeps as the rule.  Pinned by hand-written vectors in tests/test_where.py; the GPU
tests take every expected value from here, never from the code under test."""


def verdicts(recs, where):
    """per record: True (kept), False (well-formed, rejected), None (bad)"""
    return [where.keeps(v) for _, v in recs]


def filter_records(recs, where, seg_off=None):
    """mtblx_where_plan / _emit over `recs` ([(key, value)]) -> dict:
       records    the kept records in their order
       src_idx    their indices in recs
       seg_end    per segment, the END index in the kept order ([] without seg_off)
       seg_bad    per segment, the bad values
       totals     [kept, kept key bytes, kept value bytes, bad, rejected]"""
    n = len(recs)
    vd = verdicts(recs, where)
    idx = [i for i in range(n) if vd[i] is True]
    kept = [recs[i] for i in idx]
    seg_end, seg_bad = [], []
    if seg_off is not None:
        off = [int(x) for x in seg_off]
        assert off[0] == 0 and off[-1] == n and all(a <= b for a, b in zip(off, off[1:])), "the test's own seg_off"
        for q in range(len(off) - 1):
            seg_end.append(sum(1 for i in idx if i < off[q + 1]))
            seg_bad.append(sum(1 for i in range(off[q], off[q + 1]) if vd[i] is None))
    nbad = sum(1 for x in vd if x is None)
    return dict(records=kept, src_idx=idx, seg_end=seg_end, seg_bad=seg_bad,
                totals=[len(kept), sum(len(k) for k, _ in kept), sum(len(v) for _, v in kept), nbad,
                        n - len(kept) - nbad])


def segments(m, q):
    """segment q's kept records of a filter_records result"""
    lo = m["seg_end"][q - 1] if q else 0
    return m["records"][lo: m["seg_end"][q]]
