"""The yardstick of tests/test_select.py and tests/test_select_gpu.py: the Merger's set operations
(include/mtblx.h "Set operations") restated on top of merger_model.multi_iter.

The reference has no set operations, so the model is the definition itself, kept apart from the
kernel: every value is tagged with the source it came from, the reference's MultiIter (the
empty-key quirk is the model's) groups them, the tags of a group are OR-ed into its source mask,
Select.keeps decides, and the tags come off again.  The values of a kept group are put in source
order, which is what this library promises on top of the reference (merger_model.canon compares
the rest).
"""
import merger_model as mm


def _tag(sources):
    return [[(k, (s, v)) for k, v in recs] for s, recs in enumerate(sources)]


def masked_groups(sources):
    """[(key, mask, [values in source order])] of MultiIter over `sources` (lists of sorted records)"""
    out = []
    for k, tagged in mm.multi_iter(_tag(sources)):
        mask = 0
        for s, _ in tagged:
            mask |= 1 << s
        out.append((k, mask, [v for _, v in sorted(tagged, key=lambda t: t[0])]))
    return out


def select_groups(sources, sel):
    """MultiIter's items that `sel` keeps: [(key, [values in source order])]"""
    return [(k, vs) for k, mask, vs in masked_groups(sources) if sel is None or sel.keeps(mask)]


def select_merge(sources, sel, merge):
    """MergerIter's items that `sel` keeps: merge is never called for a group of one"""
    return [(k, vs[0] if len(vs) == 1 else merge(k, vs)) for k, vs in select_groups(sources, sel)]


def left_out(sources, sel):
    """(groups, records) the selection leaves out: totals[6] and [7] of the _select plans"""
    out = [(k, vs) for k, mask, vs in masked_groups(sources) if not sel.keeps(mask)]
    return len(out), sum(len(vs) for _, vs in out)
