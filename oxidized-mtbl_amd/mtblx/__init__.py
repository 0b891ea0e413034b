"""mtblx — MI355X-native mtbl block codec (drop-in for Kerollmops/oxidized-mtbl's block decode path).

Package layout
  _lib.py     ctypes binding of libmtblx.so (include/mtblx.h, include/mtblx_host.h)
  codec.py    device batch decode (HIP kernels in csrc/decode.hip)
  writer.py   Writer / WriterBuilder mirror of src/writer.rs
  synth.py    deterministic synthetic workloads of BASELINE.json's configs
  merger.py   Merger / MergerBuilder mirror of src/merger.rs over the device merge (csrc/merge.hip);
              Merger.scan_batch / get_batch: batched reads of the merged view (csrc/merge_seg.hip)
  sorter.py   Sorter / SorterBuilder mirror of src/sorter.rs over the device sort (csrc/sort.hip)
  reduce.py   Reduce / MergeError: u64 sum / min / max merge functions evaluated on the device (csrc/reduce_dev.h)
  setops.py   Select / diff_files: set operations on the Merger, a key kept by which sources hold it
              (csrc/merge_dev.h k_group_select)
  rollup.py   GroupBy / rollup_records / Rollup: records grouped by a key prefix, one aggregate per group
              (csrc/rollup.hip); Reader.rollup / rollup_batch and Merger.rollup / rollup_batch sit on it
  where.py    Where / filter_records / Filtered / filter_file: records kept or dropped by the fields of their
              value (csrc/where.hip)
"""
from ._lib import EXPORTS, LIB_PATH, lib  # noqa: F401
from .reduce import MergeError, Reduce, ReduceBatch, reduce_segments  # noqa: F401
from .rollup import GroupBy, Rollup, reduce_encode, rollup_records  # noqa: F401
from . import setops  # noqa: F401
from .setops import Select  # noqa: F401
from . import where  # noqa: F401
from .where import Filtered, Where, filter_records  # noqa: F401
from .writer import CompressionType, OutOfOrderKey, Writer, WriterBuilder  # noqa: F401


def __getattr__(name):   # Merger / MergerBuilder / Sorter / SorterBuilder need torch: imported on first use
    if name in ("Merger", "MergerBuilder", "MergedScanBatch", "merge_segments"):
        from . import merger
        return getattr(merger, name)
    if name in ("Sorter", "SorterBuilder"):
        from . import sorter
        return getattr(sorter, name)
    raise AttributeError(name)


__all__ = ["Writer", "WriterBuilder", "CompressionType", "OutOfOrderKey", "Merger", "MergerBuilder", "Sorter", "SorterBuilder",
           "MergedScanBatch", "merge_segments", "Select", "setops",
           "Reduce", "MergeError", "GroupBy", "Rollup", "rollup_records", "reduce_encode",
           "Where", "Filtered", "filter_records", "where", "lib", "LIB_PATH", "EXPORTS"]
