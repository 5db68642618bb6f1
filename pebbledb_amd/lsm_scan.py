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
list the caller passes, in iterator order, and with ``memtables=[active, *immutables]`` the
``DeviceMemTable``s whose iterators ``LsmStorage.scan`` puts in front of the tables'
(``pbf_mt_scan_size`` / ``pbf_mt_scan``, csrc/memtable_read_kernels.hpp): a memtable's range has
the semantics above (``device_memtable``'s docstring names the divergence from the reference's
``MemTable.scan``).  ``memtables=()`` is the scan over tables alone.

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
MAX_SOURCES = 64        # memtables + tables of one call


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


def _size(hs, nt: int, b: _Bounds, segments: bool, mts=None, nm: int = 0):
    """pbf_sst_scan_size (pbf_mt_scan_size with `nm` memtables in front): (records, key bytes,
    value bytes) in range before de-duplication, and with `segments` the windows (lo uint32[Q, M +
    T], hi uint32[Q, M + T])."""
    n, kb, vb = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    lo = hi = None
    if segments:
        lo = np.zeros((b.n, nm + nt), dtype=np.uint32)
        hi = np.zeros((b.n, nm + nt), dtype=np.uint32)
    out = (_vp(lo.ctypes.data) if segments and lo.size else None, _vp(hi.ctypes.data) if segments and hi.size else None,
           ctypes.byref(n), ctypes.byref(kb), ctypes.byref(vb))
    if nm:
        _native.check(_native.lib().pbf_mt_scan_size(mts, nm, hs, nt, *b.args(), *out), "pbf_mt_scan_size")
    else:
        _native.check(_native.lib().pbf_sst_scan_size(hs, nt, *b.args(), *out), "pbf_sst_scan_size")
    return n.value, kb.value, vb.value, lo, hi


def _sources(tables, memtables):
    """(tables, table handles, memtable handles, M) of one call: with memtables the table list may
    be empty and M + T is at most 64."""
    memtables = list(memtables)
    if not memtables:
        tables = _table_list(tables, "scan")
        return tables, _handles(tables), None, 0
    from .device_memtable import _mt_handles

    tables = list(tables)
    if tables:
        tables = _table_list(tables, "scan")  # the same checks and wording as without memtables
    if len(memtables) + len(tables) > MAX_SOURCES:
        raise ValueError(f"a scan takes at most {MAX_SOURCES} memtables and tables together, got "
                         f"{len(memtables)} + {len(tables)}")
    if tables and tables[0].device != memtables[0].device:
        raise ValueError("the memtables and tables of one call must share a device")
    return tables, _handles(tables) if tables else None, _mt_handles(memtables), len(memtables)


def scan_ranges(tables: Sequence, ranges, memtables=()) -> tuple[PackedRecords, np.ndarray]:
    """The batched scan: `ranges` = [(lower, upper), ...]; returns (run, range_offsets
    uint64[Q + 1]), range q = records [range_offsets[q], range_offsets[q + 1]) of the run, each
    range what ``scan_tables(tables, lower, upper)`` gives.  Ranges may overlap, repeat and come
    in any order; a record in two ranges appears in both.  At most 64 tables, all open, distinct
    and on one device, and at most 2**22 ranges x tables (ValueError otherwise).  `memtables`:
    up to 16 ``DeviceMemTable``s whose records come before the tables' (memtables[0] first); the
    table list may then be empty, memtables + tables <= 64 and ranges x (memtables + tables) <=
    2**22."""
    tables, hs, mts, nm = _sources(tables, memtables)
    b = _Bounds(ranges)
    n, kbytes, vbytes, _, _ = _size(hs, len(tables), b, False, mts, nm)
    out = _RunOut(n, kbytes, vbytes)
    ro = np.zeros(b.n + 1, dtype=np.uint64)
    if nm:
        rc = _native.lib().pbf_mt_scan(mts, nm, hs, len(tables), *b.args(), *out.args(), _vp(ro.ctypes.data), 0, None)
        _native.check(rc, "pbf_mt_scan")
    else:
        rc = _native.lib().pbf_sst_scan(hs, len(tables), *b.args(), *out.args(), _vp(ro.ctypes.data), 0, None)
        _native.check(rc, "pbf_sst_scan")
    return out.records(), ro


def scan_tables(tables: Sequence, lower: str, upper: str, memtables=()) -> PackedRecords:
    """``MergingIterator([m.scan(lower, upper) for m in memtables] + [t.scan(lower, upper) for t in
    tables])`` as a packed run (see the module docstring): one range of ``scan_ranges``."""
    return scan_ranges(tables, [(lower, upper)], memtables)[0]


def count_ranges(tables: Sequence, ranges, memtables=()) -> np.ndarray:
    """int64[Q, M + T]: the records of source u in range q (before any de-duplication across
    sources), the memtables' columns first, then the tables'.  One ``pbf_sst_scan_size`` /
    ``pbf_mt_scan_size`` call: two searches per entry, no record is copied."""
    tables, hs, mts, nm = _sources(tables, memtables)
    b = _Bounds(ranges)
    _, _, _, lo, hi = _size(hs, len(tables), b, True, mts, nm)
    return hi.astype(np.int64) - lo.astype(np.int64)
