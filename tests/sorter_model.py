"""A small Python restatement of the reference's Sorter (src/sorter.rs) over tests/merger_model.py,
the yardstick of tests/test_sorter.py and tests/test_sorter_gpu.py.

Written from the reference line by line:
    SorterBuilder::new / max_memory / max_nb_chunks / build   src/sorter.rs:25-70, src/lib.rs:11-15
    Sorter::insert with the memory rule                        :120-140
    Sorter::write_chunk                                        :142-197
    Sorter::merge_chunks                                       :199-233
    Sorter::into_iter                                          :244-257

`sort_unstable_by` (:152) is restated as Python's stable `sorted`: one of the orders the reference
allows, and exactly the order this library promises.  Chunks are record lists: writing them to
compressed temp files and reading them back changes nothing the model needs.  `entries.capacity()`
(:131) is emulated: Vec::with_capacity(131 072), doubled when a push finds the Vec full, kept by
drain(..).  That doubling is std's current amortised growth, an implementation detail of the
standard library rather than a documented guarantee (as the oracle notes for its own Vec
capacity emulation).
"""
import merger_model as mm

DEFAULT_NB_CHUNKS, MIN_NB_CHUNKS = 25, 1                              # src/lib.rs:11-12
DEFAULT_SORTER_MEMORY, MIN_SORTER_MEMORY = 1_073_741_824, 10_485_760  # :13-14
INITIAL_SORTER_VEC_SIZE = 131_072                                     # :15
ENTRY_SIZE = 32   # size_of::<Entry>() on 64-bit: Vec<u8> (ptr, cap, len) + key_len: usize (:72-75)


class Sorter:
    def __init__(self, merge, max_memory=DEFAULT_SORTER_MEMORY, max_nb_chunks=DEFAULT_NB_CHUNKS):
        self.merge = merge
        self.max_memory = max(max_memory, MIN_SORTER_MEMORY)       # :37
        self.max_nb_chunks = max(max_nb_chunks, MIN_NB_CHUNKS)     # :44
        self.chunks = []                                           # :60
        self.entries = []                                          # :61
        self.capacity = INITIAL_SORTER_VEC_SIZE                    # :61 with_capacity
        self.entry_bytes = 0                                       # :62
        self.chunk_sizes, self.merges, self.cuts = [], 0, []       # for the tests: records per write_chunk,
        self.inserted = 0                                          # merge_chunks runs, the inserts that cut

    def insert(self, key, val):
        self.inserted += 1
        self.entry_bytes += len(key) + len(val)                    # :127-128
        if len(self.entries) == self.capacity:                     # :129 push on a full Vec: amortised doubling
            self.capacity *= 2
        self.entries.append((bytes(key), bytes(val)))
        entries_vec_size = self.capacity * ENTRY_SIZE              # :131
        if self.entry_bytes + entries_vec_size >= self.max_memory:  # :132
            self.cuts.append(self.inserted)
            self.write_chunk()                                     # :133
            if len(self.chunks) > self.max_nb_chunks:              # :134
                self.merge_chunks()                                # :135

    def _merged(self, key, vals):
        return vals[0] if len(vals) == 1 else self.merge(key, vals)   # :166-170, :182-186

    def write_chunk(self):
        self.chunk_sizes.append(len(self.entries))
        out = []
        entries = sorted(self.entries, key=lambda e: e[0])         # :152 (stable: see the module docstring)
        self.entries = []                                          # :155 drain(..): the capacity stays
        current = None                                             # :154
        for key, val in entries:
            if current is None:                                    # :157-161
                current = (key, [val])
            elif current[0] == key:                                # :163-164
                current[1].append(val)
            else:                                                  # :165-176
                out.append((current[0], self._merged(*current)))
                current = (key, [val])
        if current is not None:                                    # :181-188
            out.append((current[0], self._merged(*current)))
        self.chunks.append(out)                                    # :191
        self.entry_bytes = 0                                       # :192

    def merge_chunks(self):
        self.merges += 1
        self.chunks = [mm.merge_iter(self.chunks, self.merge)]     # :211-228

    def into_iter(self):
        self.write_chunk()                                         # :246
        return mm.merge_iter(self.chunks, self.merge)              # :253-256


def run(records, merge, **kw):
    """insert every record, then into_iter -> ([(key, merged)], the Sorter)"""
    s = Sorter(merge, **kw)
    for k, v in records:
        s.insert(k, v)
    return s.into_iter(), s


def concat_any(_key, values):
    """b"".join, also for one value (the built-in "concat" of the device path)"""
    return b"".join(values)
