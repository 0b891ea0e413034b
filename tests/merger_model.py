"""A small Python restatement of the reference's MergerIter / MultiIter (src/merger.rs), the
yardstick of tests/test_merger.py and tests/test_merger_gpu.py.

Written from the reference line by line:
    Entry::new / fill                 src/merger.rs:13-43    one pending record per source
    Ord for Entry: the key only       :45-49
    into_merge_iter / into_iter       :108-142               a BinaryHeap<Reverse<Entry>> of the sources' first records
    MergerIter::next                  :172-213
    MultiIter::next                   :226-259
including the empty-key quirk of :182-186 / :236-240: `cur_key.is_empty()` doubles as "no current
key", so after an empty-key record has been taken, the next heap entry's key is adopted again and
`cur_vals.clear()` runs again.

The heap is Python's heapq over (key, tick, source): equal keys come out in push order here, which
is ONE of the orders the reference's BinaryHeap may produce (std leaves the order of equal
elements unspecified).  So a comparison against this model uses the key sequence and the multiset
of values per key (`canon`), never the order inside a group.

Sources are .mtbl files: their records come from pyoracle.file_scan, and files are made with
pyoracle.write_file (oracle/ is used as it is).
"""
import heapq

import pyoracle


def make_source(records, block_size=1024, restart_interval=16) -> bytes:
    """a sorted record list -> .mtbl bytes by the oracle Writer"""
    return pyoracle.write_file(records, block_size, restart_interval)


def source_records(file_bytes: bytes):
    r = pyoracle.file_scan(file_bytes)
    assert r["end"] == 0, r
    return r["records"]


class _Heap:
    """the BinaryHeap<Reverse<Entry>> of :109-115 with Entry::fill (:29-42)"""

    def __init__(self, sources):
        self.iters = [iter(s) for s in sources]
        self.h = []
        self.tick = 0
        for i in range(len(self.iters)):   # :110-115 Entry::new fills; an exhausted source is not pushed
            self._fill(i)

    def _fill(self, i):
        rec = next(self.iters[i], None)
        if rec is not None:
            self.tick += 1
            heapq.heappush(self.h, (rec[0], self.tick, i, rec[1]))

    def peek(self):
        return self.h[0] if self.h else None

    def take(self):
        """:189-193: mem::take the value, fill the entry again, pop it if its source is exhausted"""
        k, _, i, v = heapq.heappop(self.h)
        self._fill(i)
        return v


def _next(heap):
    """the common loop of MergerIter::next (:173-197) and MultiIter::next (:227-251)
    -> (pending, cur_key, cur_vals)"""
    cur_key, cur_vals, pending = b"", [], False   # :173-174 clear(); pending is false between calls (:208, :254)
    while True:
        e = heap.peek()                           # :177-180
        if e is None:
            break
        if len(cur_key) == 0:                     # :182 cur_key.is_empty()
            cur_key = e[0]                        # :183
            cur_vals = []                         # :184
            pending = True                        # :185
        if cur_key == e[0]:                       # :188
            cur_vals.append(heap.take())          # :189-193
        else:
            break                                 # :195
    return pending, cur_key, cur_vals


def multi_iter(sources):
    """MultiIter (:216-260): [(key, [values])]"""
    heap, out = _Heap(sources), []
    while True:
        pending, k, vs = _next(heap)
        if not pending:                           # :253-258
            return out
        out.append((k, vs))


def merge_iter(sources, merge):
    """MergerIter (:159-214): [(key, merged)]; merge is never called for a group of one (:200-207)"""
    heap, out = _Heap(sources), []
    while True:
        pending, k, vs = _next(heap)
        if not pending:                           # :199, :210-212
            return out
        out.append((k, vs[0] if len(vs) == 1 else merge(k, vs)))


def concat(_key, values):
    """the merge function of the reference's own tests (src/merger.rs:269-275, src/sorter.rs:266-269)"""
    assert len(values) != 1
    return b"".join(values)


def canon(groups):
    """what the reference fixes of a MultiIter result: the key sequence and each key's multiset of values"""
    return [(k, sorted(vs)) for k, vs in groups]


def easy_sources():
    """src/merger.rs:277-287: source i holds keys {:010} for i .. 30 * (i + 1); the value is the
    key repeated i / 10_000 times, i.e. empty"""
    return [[(b"%010d" % j, (b"%010d" % j) * (j // 10_000)) for j in range(i, 30 * (i + 1))] for i in range(10)]
