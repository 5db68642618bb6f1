"""Compaction over SSTables resident on the device: the record run that
``force_compaction_l0`` / ``force_compaction_l1_or_more_level`` (reference
src/lsm_storage.py:253-294) feed to ``_compact``, produced from ``DeviceSSTable``s without the
reference's iterators, and the output SSTable files built from it.

``merge_tables`` is ``MergingIterator([SSTableIterator(t) for t in tables])``
(src/iterators.py:110-190): every distinct key in ascending order, each with the record of the
lowest table index that stores it (``tables[0]`` is the first iterator; the heap key is
``(key, iterator_index)`` and ``_filter_duplicate_keys`` keeps the first record of a key).  An
empty value is a value like any other: the reference has no tombstones.  ``concat_tables`` is
``ConcatenatingIterator`` (iterators.py:193-207): every record, table after table in list order.
Both are one ``pbf_sst_merge`` call (csrc/sstable_merge_kernels.hpp): a merge by rank — every
input record finds its place with one lower-bound search per other table — then scans over the
ranked records and one packed copy of the kept keys and values.

Keys order as unsigned bytes, which is the reference's ``str`` order for the keys a resident
table can hold (``DeviceSSTable`` refuses the non-ASCII keys the reference cannot read back).

``compact_l0`` / ``compact_level`` are the merge / concatenation followed by
``sstable_data.build_sstables``: the files ``_compact`` writes, without the state update and the
manifest event, which stay with the caller.  ``compact_l0_resident`` / ``compact_level_resident``
are the same compactions with the run kept on the device and the outputs opened there as
``DeviceSSTable``s (``resident_write``; include/pebblebloom.h "Resident write path").
"""
from __future__ import annotations

import ctypes
from typing import Sequence

import numpy as np

from . import _native
from .keys import PackedKeys, PackedRecords
from .sstable_data import BLOCK_SIZE, _check_block_size, _check_max_sstable_size, build_sstables
from .sstable_read import _handles

_vp = ctypes.c_void_p
MAX_TABLES = 64  # kSstTablesPerLaunch: the tables travel in one kernel's arguments


def _bounds(tables) -> tuple[int, int]:
    """(records, key + value bytes) of the tables together, from host-known sizes: a data section
    is its records (8 bytes of sizes each, then key and value), one u16 per record and one u16
    per block."""
    n = nbytes = 0
    nb, nr, dl = ctypes.c_uint32(), ctypes.c_uint64(), ctypes.c_uint64()
    for t in tables:
        _native.check(_native.lib().pbf_sst_info(t._h, ctypes.byref(nb), ctypes.byref(nr), ctypes.byref(dl)),
                      "pbf_sst_info")
        n += nr.value
        nbytes += dl.value - 10 * nr.value - 2 * nb.value
    return n, nbytes


def _table_list(tables, what: str) -> list:
    """The tables of one merge or scan (`what`) as a list."""
    tables = list(tables)
    if not tables:
        raise ValueError(f"no tables to {what}")
    if len(tables) > MAX_TABLES:
        raise ValueError(f"a {what} takes at most {MAX_TABLES} tables, got {len(tables)}")
    return tables


class _RunOut:
    """Host arrays for a record run of at most `n` records, `kbytes` key bytes and `vbytes` value
    bytes, as ``pbf_sst_merge`` and ``pbf_sst_scan`` fill them."""

    def __init__(self, n: int, kbytes: int, vbytes: int):
        self.keys = np.empty(kbytes, dtype=np.uint8)
        self.values = np.empty(vbytes, dtype=np.uint8)
        self.ko = np.empty(n + 1, dtype=np.uint64)
        self.vo = np.empty(n + 1, dtype=np.uint64)
        self.n_out, self.kb, self.vb = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()

    def args(self):
        """keys_out ... value_bytes_out of either call."""
        return (_vp(self.keys.ctypes.data) if self.keys.size else None, self.keys.size, _vp(self.ko.ctypes.data),
                _vp(self.values.ctypes.data) if self.values.size else None, self.values.size, _vp(self.vo.ctypes.data),
                self.ko.size, ctypes.byref(self.n_out), ctypes.byref(self.kb), ctypes.byref(self.vb))

    def records(self) -> PackedRecords:
        """The run the call wrote."""
        m = self.n_out.value
        pk = PackedKeys(self.keys[:self.kb.value], m, offsets=self.ko[:m + 1])
        return PackedRecords(pk, self.values[:self.vb.value], self.vo[:m + 1])


def _run(tables: Sequence, mode: int) -> PackedRecords:
    tables = _table_list(tables, "merge")
    hs = _handles(tables)
    n, nbytes = _bounds(tables)
    out = _RunOut(n, nbytes, nbytes)
    _native.check(_native.lib().pbf_sst_merge(hs, len(tables), mode, *out.args(), 0, None), "pbf_sst_merge")
    return out.records()


def merge_tables(tables: Sequence) -> PackedRecords:
    """``MergingIterator`` over the tables' ``SSTableIterator``s as a packed run (see the module
    docstring).  At most 64 tables, all open, distinct and on one device (ValueError otherwise)."""
    return _run(tables, _native.PBF_MERGE_DEDUP)


def concat_tables(tables: Sequence) -> PackedRecords:
    """``ConcatenatingIterator`` over the tables' ``SSTableIterator``s as a packed run: every
    record in list order, also where the tables overlap or are out of order."""
    return _run(tables, _native.PBF_MERGE_CONCAT)


def compact_l0(tables: Sequence, max_sstable_size: int = 262_144_000, block_size: int = BLOCK_SIZE,
               fp_rate: float = 0.001, device=None):
    """``force_compaction_l0`` (lsm_storage.py:253-260) up to the files: ``merge_tables`` then
    ``build_sstables``; returns what ``build_sstables`` returns, (outputs, records written).

    The merged run makes one host round trip between the two calls: ``merge_tables`` brings it to
    host memory and ``build_sstables`` uploads it again (``pbf_build_sstables`` reads host
    memory)."""
    tables = list(tables)
    run = merge_tables(tables)
    return build_sstables(run, None, max_sstable_size, block_size, fp_rate, tables[0].device if device is None else device)


def compact_level(tables: Sequence, max_sstable_size: int = 262_144_000, block_size: int = BLOCK_SIZE,
                  fp_rate: float = 0.001, device=None):
    """``force_compaction_l1_or_more_level`` (lsm_storage.py:272-284) up to the files:
    ``concat_tables`` then ``build_sstables``, with the same host round trip as ``compact_l0``."""
    tables = list(tables)
    run = concat_tables(tables)
    return build_sstables(run, None, max_sstable_size, block_size, fp_rate, tables[0].device if device is None else device)


def _compact_resident(tables, mode: int, max_sstable_size: int, block_size: int, fp_rate: float):
    from .resident_write import finish_job

    tables = _table_list(tables, "merge")
    _check_block_size(block_size)
    _check_max_sstable_size(max_sstable_size)
    hs = _handles(tables)
    job, nt, written = _vp(), ctypes.c_uint64(), ctypes.c_uint64()
    _native.check(_native.lib().pbf_compact_begin(hs, len(tables), mode, block_size, max_sstable_size,
                                                  ctypes.byref(job), ctypes.byref(nt), ctypes.byref(written)),
                  "pbf_compact_begin")
    return finish_job(job, nt.value, fp_rate, tables[0].device), written.value


def compact_l0_resident(tables: Sequence, max_sstable_size: int = 262_144_000, block_size: int = BLOCK_SIZE,
                        fp_rate: float = 0.001):
    """``compact_l0`` without the host: the merged run stays on the device, where it is planned
    (csrc/sstable_plan_kernels.hpp), encoded, filtered and opened.  Returns (outputs as
    ``DeviceSSTable``s in the order ``_compact`` returns them, records written); each output's
    ``to_bytes()`` is the file ``compact_l0`` returns for it.  Arguments and refusals are
    ``compact_l0``'s; no output gives ``([], written)``.  The inputs may be closed as soon as the
    call returns."""
    return _compact_resident(tables, _native.PBF_MERGE_DEDUP, max_sstable_size, block_size, fp_rate)


def compact_level_resident(tables: Sequence, max_sstable_size: int = 262_144_000, block_size: int = BLOCK_SIZE,
                           fp_rate: float = 0.001):
    """``compact_level`` without the host, as ``compact_l0_resident``."""
    return _compact_resident(tables, _native.PBF_MERGE_CONCAT, max_sstable_size, block_size, fp_rate)
