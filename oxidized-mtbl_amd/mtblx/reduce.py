"""Device merge functions: u64 sum / min / max over fixed-width fields (include/mtblx.h "Device merge
functions", csrc/reduce_dev.h).

    Reduce("sum")                    one little-endian u64 per value, added mod 2^64
    Reduce("sum", "min", "max")      24-byte values: (count, time_first, time_last)
    "sum_u64" | "min_u64" | "max_u64"   shorthands for one field

A Reduce is accepted wherever the Merger and the Sorter accept "concat": the groups are then reduced
on the device (mtblx_merge_emit_reduce / mtblx_sort_emit_reduce) and no record returns to the host.
It is not callable on purpose: a callable merge function is the host path.  ``Reduce.host`` is the
same function on the host, for documentation and A/B runs.

As the reference never calls its merge function for a group of one (src/merger.rs:200-201,
src/sorter.rs:166-167), a value alone in its group comes out unchanged whatever its length; in a
group of two or more every value must be exactly 8 * nfields bytes long, else MergeError.
"""
from __future__ import annotations

OPS = {"sum": 0, "min": 1, "max": 2}          # MTBLX_REDUCE_SUM / _MIN / _MAX
MAX_FIELDS = 8                                 # MTBLX_REDUCE_MAX_FIELDS
SHORTHANDS = {"sum_u64": "sum", "min_u64": "min", "max_u64": "max"}
_MASK = (1 << 64) - 1


class MergeError(RuntimeError):
    """the merge function failed (the reference's Error::Merge): a group of two or more holds a
    value that is not 8 * nfields bytes long (MTBLX_MERGE_BADVALUE)"""


class Reduce:
    """1 to 8 fields, each an unsigned 64-bit little-endian integer with one op: "sum" | "min" | "max" """

    def __init__(self, *ops: str):
        if not 1 <= len(ops) <= MAX_FIELDS:
            raise ValueError(f"Reduce takes 1 to {MAX_FIELDS} ops, not {len(ops)}")
        for op in ops:
            if op not in OPS:
                raise ValueError(f"Reduce op: {op!r} (one of 'sum', 'min', 'max')")
        self.ops = tuple(ops)

    @property
    def width(self) -> int:
        return 8 * len(self.ops)

    def __repr__(self):
        return "Reduce(" + ", ".join(repr(o) for o in self.ops) + ")"

    def __eq__(self, other):
        return isinstance(other, Reduce) and other.ops == self.ops

    def __hash__(self):
        return hash(self.ops)

    def cstruct(self):
        """the mtblx_reduce of this spec"""
        from . import _lib
        r = _lib.ReduceSpec()
        r.nfields = len(self.ops)
        for f, op in enumerate(self.ops):
            r.op[f] = OPS[op]
        return r

    def host(self, key, values) -> bytes:
        """the same merge function on the host, as a callable(key, values) -> bytes would be given"""
        w = self.width
        for v in values:
            if len(v) != w:
                raise MergeError(f"merge: a value of {len(v)} bytes in a group of {len(values)}, {w} expected")
        out = bytearray()
        for f, op in enumerate(self.ops):
            xs = [int.from_bytes(v[8 * f: 8 * f + 8], "little") for v in values]
            x = sum(xs) & _MASK if op == "sum" else min(xs) if op == "min" else max(xs)
            out += x.to_bytes(8, "little")
        return bytes(out)


def as_reduce(merge):
    """a Reduce or one of its shorthand names -> the Reduce; anything else -> None"""
    if isinstance(merge, Reduce):
        return merge
    if isinstance(merge, str) and merge in SHORTHANDS:
        return Reduce(SHORTHANDS[merge])
    return None


def check_merge(merge):
    """what the builders accept: a built-in name, a Reduce (shorthands become one), a callable"""
    r = as_reduce(merge)
    if r is not None:
        return r
    if not callable(merge) and merge not in ("concat", "first", "last"):
        raise ValueError(f"merge: {merge!r}")
    return merge
