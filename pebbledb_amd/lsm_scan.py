"""Range scan over SSTables resident on the device: ``SSTable.scan(lower, upper)`` (reference
src/sstable.py:189, the bounded ``SSTableIterator`` of src/iterators.py:58-141) and the
``MergingIterator`` over those that ``LsmStorage.scan`` yields from (src/lsm_storage.py:187-190),
for one range or a batch of ranges.

Semantics kept from the reference:

* a range is ``lower <= key <= upper``, inclusive at both ends, in key order; ``lower > upper``
  yields nothing; ``lower == ""`` starts at the table's first record;
* ``upper == ""`` means NO upper bound (``DataBlockIterator.__next__`` tests ``if self._end_key
  and ...``): ``scan("k0150", "")`` is everything from ``k0150`` on;
* over several tables every distinct key in range appears once, ascending, with the record of the
  lowest table index that stores it (``tables[0]`` is the first iterator, as in
  ``compaction.merge_tables``); an empty value is a value.

``LsmStorage.scan`` reads the memtables and level 0 only.  The calls here take whatever table
list the caller passes, in iterator order; the memtable iterators stay with the caller, as they
do for ``lsm_get.get_batch``.

Bounds are ``str`` and compare as their UTF-8 bytes against the stored key bytes, which is
Python's ``str`` order (code points) for the ASCII keys a resident table holds; a non-ASCII bound
is simply a position between keys.

Divergence (an input the reference mishandles): ``SSTableIterator.__next__`` recurses once per
consecutive block that yields nothing, so a bounded scan over a table with about 1000 or more
consecutive out-of-range blocks raises ``RecursionError`` there.  Here the records are returned.

``scan_ranges`` is one ``pbf_sst_scan_size`` call (the windows' sizes, which bound the run) and
one ``pbf_sst_scan`` call (csrc/sstable_scan_kernels.hpp): one lower-bound pair per (range,
table), then the rank merge of ``compaction.merge_tables`` restricted to those windows, every
range in the same launches.
"""
from __future__ import annotations

import ctypes
from typing import Sequence

import numpy as np

from . import _native
from .compaction import _RunOut, _table_list
from .keys import PackedRecords
from .sstable_read import _handles

_vp = ctypes.c_void_p
MAX_SEGMENTS = 1 << 22  # PBF_SCAN_MAX_SEGMENTS: ranges x tables of one call


class _Bounds:
    """The ranges of one call, packed as the library reads them."""

    def __init__(self, ranges):
        ranges = list(ranges)
        lows, ups = [], []
        for r in ranges:
            lower, upper = r
            for b in (lower, upper):
                if not isinstance(b, str):
                    raise ValueError(f"a scan bound must be a str, got {b!r}: for every record of a table use "
                                     "DeviceSSTable.records() / merge_tables (\"\" as upper means no upper bound)")
            lows.append(lower.encode("utf-8"))
            ups.append(upper.encode("utf-8"))
        self.n = len(ranges)
        self.open = np.array([len(u) == 0 for u in ups], dtype=np.uint8)
        self.lower, self.lower_offsets = self._pack(lows)
        self.upper, self.upper_offsets = self._pack(ups)

    @staticmethod
    def _pack(bs):
        offs = np.zeros(len(bs) + 1, dtype=np.uint64)
        if bs:
            np.cumsum([len(b) for b in bs], out=offs[1:])
        return np.frombuffer(b"".join(bs) or b"\0", dtype=np.uint8), offs

    def args(self):
        return (_vp(self.lower.ctypes.data), _vp(self.lower_offsets.ctypes.data), _vp(self.upper.ctypes.data),
                _vp(self.upper_offsets.ctypes.data), _vp(self.open.ctypes.data) if self.n else None, self.n)


def _size(hs, nt: int, b: _Bounds, segments: bool):
    """pbf_sst_scan_size: (records, key bytes, value bytes) in range before de-duplication, and
    with `segments` the windows (lo uint32[Q, T], hi uint32[Q, T])."""
    n, kb, vb = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    lo = hi = None
    if segments:
        lo = np.zeros((b.n, nt), dtype=np.uint32)
        hi = np.zeros((b.n, nt), dtype=np.uint32)
    rc = _native.lib().pbf_sst_scan_size(hs, nt, *b.args(), _vp(lo.ctypes.data) if segments and lo.size else None,
                                         _vp(hi.ctypes.data) if segments and hi.size else None, ctypes.byref(n),
                                         ctypes.byref(kb), ctypes.byref(vb))
    _native.check(rc, "pbf_sst_scan_size")
    return n.value, kb.value, vb.value, lo, hi


def scan_ranges(tables: Sequence, ranges) -> tuple[PackedRecords, np.ndarray]:
    """The batched scan: `ranges` = [(lower, upper), ...]; returns (run, range_offsets
    uint64[Q + 1]), range q = records [range_offsets[q], range_offsets[q + 1]) of the run, each
    range what ``scan_tables(tables, lower, upper)`` gives.  Ranges may overlap, repeat and come
    in any order; a record in two ranges appears in both.  At most 64 tables, all open, distinct
    and on one device, and at most 2**22 ranges x tables (ValueError otherwise)."""
    tables = _table_list(tables, "scan")
    b = _Bounds(ranges)
    hs = _handles(tables)
    n, kbytes, vbytes, _, _ = _size(hs, len(tables), b, False)
    out = _RunOut(n, kbytes, vbytes)
    ro = np.zeros(b.n + 1, dtype=np.uint64)
    rc = _native.lib().pbf_sst_scan(hs, len(tables), *b.args(), *out.args(), _vp(ro.ctypes.data), 0, None)
    _native.check(rc, "pbf_sst_scan")
    return out.records(), ro


def scan_tables(tables: Sequence, lower: str, upper: str) -> PackedRecords:
    """``MergingIterator([t.scan(lower, upper) for t in tables])`` as a packed run (see the module
    docstring): one range of ``scan_ranges``."""
    return scan_ranges(tables, [(lower, upper)])[0]


def count_ranges(tables: Sequence, ranges) -> np.ndarray:
    """int64[Q, T]: the records of table t in range q (before any de-duplication across tables).
    One ``pbf_sst_scan_size`` call: two searches per entry, no record is copied."""
    tables = _table_list(tables, "scan")
    b = _Bounds(ranges)
    _, _, _, lo, hi = _size(_handles(tables), len(tables), b, True)
    return hi.astype(np.int64) - lo.astype(np.int64)
