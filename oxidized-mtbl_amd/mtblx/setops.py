"""Set operations on the Merger: keep a key by which sources hold it (include/mtblx.h "Set
operations", csrc/merge_dev.h k_group_select).

A group of the Merger holds at most one record per source, so which sources hold its key is one
64-bit mask.  A Select keeps the group iff its mask has every `require` bit, no `exclude` bit and
between `min_count` and `max_count` bits.  The empty-key quirk runs first: the selection sees the
groups the Merger yields.

    Select.union()                  the Merger as it is
    Select.intersection(nsrc)       the keys every one of nsrc sources holds
    Select.difference(keep, drop)   the keys of source `keep` that no source of `drop` holds
    Select.exactly_one()            the keys one source alone holds (two sources: symmetric difference)
    Select.at_least(k)              the keys k or more sources hold

merger.merge_records / merge_all / merge_segments take it as ``select=``, MergerBuilder.select(sel)
and Merger(..., select=sel) hand it to every Merger method.  diff_files(new, old) is the "new since
yesterday" case in one call.
"""
from __future__ import annotations

from . import _lib


def _mask(indices, what):
    if isinstance(indices, int):
        indices = (indices,)
    m = 0
    for i in indices:
        if not isinstance(i, int) or isinstance(i, bool) or i < 0 or i >= _lib.MERGE_MAX_SOURCES:
            raise ValueError(f"Select: {what} takes source indices 0..63, not {i!r}")
        m |= 1 << i
    return m


class Select:
    """The rule of mtblx_select over source indices.  `require` / `exclude`: the sources that must /
    must not hold the key; `min_count` / `max_count`: how many sources hold it (0 reads as 1; 1..64)."""

    def __init__(self, require=(), exclude=(), min_count: int = 1, max_count: int = 64):
        self.require = _mask(require, "require")
        self.exclude = _mask(exclude, "exclude")
        if self.require & self.exclude:
            raise ValueError("Select: a source is both required and excluded")
        for name, v in (("min_count", min_count), ("max_count", max_count)):
            if not isinstance(v, int) or isinstance(v, bool):
                raise ValueError(f"Select: {name} is an integer")
        if min_count < 0 or max_count < 1 or max_count > _lib.MERGE_MAX_SOURCES:
            raise ValueError("Select: 0 <= min_count, 1 <= max_count <= 64")
        self.min_count = max(min_count, 1)
        self.max_count = max_count
        if self.min_count > self.max_count:
            raise ValueError("Select: min_count > max_count")

    @classmethod
    def union(cls) -> "Select":
        return cls()

    @classmethod
    def intersection(cls, nsrc: int) -> "Select":
        if not isinstance(nsrc, int) or nsrc < 1 or nsrc > _lib.MERGE_MAX_SOURCES:
            raise ValueError("Select.intersection: 1 to 64 sources")
        return cls(require=range(nsrc))

    @classmethod
    def difference(cls, keep, drop) -> "Select":
        return cls(require=keep, exclude=drop)

    @classmethod
    def exactly_one(cls) -> "Select":
        return cls(max_count=1)

    @classmethod
    def at_least(cls, k: int) -> "Select":
        return cls(min_count=k)

    def keeps(self, mask: int) -> bool:
        """the rule itself: is a group whose sources are the bits of `mask` kept?"""
        return (mask & self.require) == self.require and not (mask & self.exclude) and \
            self.min_count <= bin(mask).count("1") <= self.max_count

    def nsrc_min(self) -> int:
        """the fewest sources the rule can be applied to: one more than the highest index it names"""
        return (self.require | self.exclude).bit_length()

    def check(self, nsrc: int) -> "Select":
        """raises ValueError where the C calls return MTBLX_E_INVAL for `nsrc` sources, or where the
        rule cannot be applied at all: more than 64 sources are merged in rounds, and a rule over
        masks cannot be applied per round"""
        if nsrc > _lib.MERGE_MAX_SOURCES:
            raise ValueError("a selection takes at most 64 sources (a rule over source masks cannot be applied per round)")
        if self.nsrc_min() > nsrc:
            raise ValueError(f"Select names source {self.nsrc_min() - 1}, but there are {nsrc} sources")
        return self

    def cstruct(self) -> "_lib.SelectSpec":
        return _lib.SelectSpec(self.require, self.exclude, self.min_count, self.max_count)

    def __eq__(self, other):
        return isinstance(other, Select) and self._t() == other._t()

    def __hash__(self):
        return hash(self._t())

    def _t(self):
        return (self.require, self.exclude, self.min_count, self.max_count)

    def __repr__(self):
        bits = lambda m: [i for i in range(64) if m >> i & 1]   # noqa: E731
        return f"Select(require={bits(self.require)}, exclude={bits(self.exclude)}, " \
               f"min_count={self.min_count}, max_count={self.max_count})"


def as_select(sel, nsrc: int):
    """None or a Select checked against `nsrc` sources"""
    if sel is None:
        return None
    if not isinstance(sel, Select):
        raise ValueError(f"select: {sel!r} is not a Select")
    return sel.check(nsrc)


def diff_files(new, old, **write_file_kwargs):
    """The .mtbl file (device uint8 tensor) of the records of `new` whose key `old` does not hold:
    "new since yesterday", on the device from the scan of the two files to the written blocks.
    `new` / `old`: a reader.Reader, or the bytes / device tensor of a .mtbl file.  Keyword arguments
    go to Merger.write_file (block_size, restart_interval, compression); ``stream=`` is the stream
    of the stream contract."""
    from . import merger, reader
    stream = write_file_kwargs.pop("stream", None)
    rs = [r if isinstance(r, reader.Reader) else reader.Reader(r) for r in (new, old)]
    return merger.Merger(rs, "first", stream, Select.difference(0, 1)).write_file(**write_file_kwargs)
