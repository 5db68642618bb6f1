"""The write path on the device: a memtable flush from a put log or a write-ahead log.

The reference's flush (``LsmStorage._do_flush``, src/lsm_storage.py:193-205) feeds
``MemTableIterator`` over a red-black tree to ``SSTableBuilder``: the puts of one memtable ordered
by key, where the last put of a key wins (the tree replaces the data of a key it already holds,
src/red_black_tree.py:118-120).  Recovery has the same shape: ``MemTable.create_from_wal``
(src/memtable.py:29-53) replays a WAL — ``Record.to_bytes()`` of every put in put order — into a
tree one insert at a time.

``sort_log`` produces that run from the packed puts in one ``pbf_log_sort`` call
(csrc/memtable_kernels.hpp): a sort of the puts by (key, put index) — tiles sorted in LDS, then
merge passes by rank — a mark of the last put of every key, and the compaction merge's scans and
packed copy.  ``flush_log`` is ``sort_log`` followed by ``sstable_data.build_sstable``: the bytes
of the ``.sst`` file ``_do_flush`` writes.  ``flush_wal`` starts from a WAL file or its bytes
(``PackedRecords.from_wal``): ``create_from_wal`` plus ``_do_flush``, without the state update and
the manifest event, which stay with the caller.  ``flush_log_resident`` / ``flush_wal_resident`` keep
the sorted run on the device and return the flushed table as an open ``DeviceSSTable``.

Keys order as unsigned bytes, which is the reference's ``str`` order for ASCII keys; a non-ASCII
key is refused, as ``DeviceSSTable`` refuses a table that stores one (the reference writes
``key_size = len(str)`` in characters, record.py:25, and cannot read such a record back).  An
empty value is a value like any other: the reference has no tombstones.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from . import _native
from .keys import PackedKeys, PackedRecords
from .sstable_data import BLOCK_SIZE, _check_block_size, build_sstable, key_offsets

_vp = ctypes.c_void_p
SORT_TILE = 2048   # kMtTile: entries one workgroup sorts in LDS
FAN_IN = 8         # kMtFanIn: runs merged into one per pass
MAX_PUTS = 2 ** 32 - 2


def merge_passes(n: int) -> int:
    """k_mt_merge_rank launches for a log of n puts."""
    passes, run = 0, SORT_TILE
    while run < n:
        run *= FAN_IN
        passes += 1
    return passes


def _as_log(puts) -> PackedRecords:
    log = puts if isinstance(puts, PackedRecords) else PackedRecords.from_iter(puts)
    if not log.ascii:
        raise ValueError("a put log with a non-ASCII key cannot be flushed: the reference writes key_size in "
                         "characters (record.py:25) and cannot read such a record back")
    return log


def _ptr(a: np.ndarray):
    return _vp(a.ctypes.data) if a.size else None


def _log_arrays(log: PackedRecords):
    """(keys, key offsets, values, value offsets) of a log as ``pbf_log_sort`` reads them."""
    return (np.ascontiguousarray(log.keys.data, dtype=np.uint8),
            np.ascontiguousarray(key_offsets(log.keys), dtype=np.uint64),
            np.ascontiguousarray(log.values, dtype=np.uint8).reshape(-1),
            np.ascontiguousarray(log.value_offsets, dtype=np.uint64))


def sort_log(puts, device=None, with_index: bool = False):
    """``MemTableIterator``'s run of a put log: every distinct key ascending, each with the value
    of its last put, as a ``PackedRecords`` (``ascii=True``).  `puts` is a ``PackedRecords`` in put
    order, or any iterable ``PackedRecords.from_iter`` takes.  With `with_index`, also the log
    index of the put every record of the run came from (uint32[n])."""
    from .bloom_filter import _default_device

    log = _as_log(puts)
    dev = _default_device if device is None else int(device)
    n = log.n
    kin, ko, vin, vo = _log_arrays(log)
    kbytes, vbytes = (int(ko[-1]), int(vo[-1])) if n else (0, 0)
    keys, values = np.empty(kbytes, dtype=np.uint8), np.empty(vbytes, dtype=np.uint8)
    oko, ovo = np.empty(n + 1, dtype=np.uint64), np.empty(n + 1, dtype=np.uint64)
    put = np.empty(n + 1, dtype=np.uint32)
    n_out, kb, vb = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    rc = _native.lib().pbf_log_sort(dev, _ptr(kin), _vp(ko.ctypes.data), _ptr(vin), _vp(vo.ctypes.data), n,
                                    _ptr(keys), keys.size, _vp(oko.ctypes.data), _ptr(values), values.size,
                                    _vp(ovo.ctypes.data), n + 1, _vp(put.ctypes.data) if with_index else None,
                                    ctypes.byref(n_out), ctypes.byref(kb), ctypes.byref(vb))
    _native.check(rc, "pbf_log_sort")
    m = n_out.value
    run = PackedRecords(PackedKeys(keys[:kb.value], m, offsets=oko[:m + 1]), values[:vb.value], ovo[:m + 1], ascii=True)
    return (run, put[:m]) if with_index else run


def flush_log(puts, block_size: int = BLOCK_SIZE, fp_rate: float = 0.001, device=None):
    """``_do_flush`` up to the file for a memtable that received `puts`: ``sort_log`` then
    ``build_sstable``; returns what ``build_sstable`` returns (file bytes, meta blocks, filter).
    An empty log behaves as ``build_sstable`` does on an empty run."""
    return build_sstable(sort_log(puts, device=device), None, block_size, fp_rate, device)


def flush_wal(wal, block_size: int = BLOCK_SIZE, fp_rate: float = 0.001, device=None):
    """``MemTable.create_from_wal`` plus ``_do_flush`` up to the file: `wal` is the path of a WAL
    file or its bytes (``PackedRecords.from_wal``), then ``flush_log``."""
    return flush_log(_wal_log(wal), block_size, fp_rate, device)


def _wal_log(wal) -> PackedRecords:
    if isinstance(wal, (str, os.PathLike)):
        with open(wal, "rb") as f:
            wal = f.read()
    return PackedRecords.from_wal(wal)


def flush_log_resident(puts, block_size: int = BLOCK_SIZE, fp_rate: float = 0.001, device=None):
    """``flush_log`` without the way back: the log goes up once, the sorted run stays on the device,
    where it is planned, encoded, filtered and opened.  Returns the ``DeviceSSTable``; its
    ``to_bytes()`` is the file ``flush_log`` returns.  An empty log raises as ``build_sstable``
    does on an empty run, a non-ASCII key as ``flush_log`` does."""
    from .bloom_filter import _default_device
    from .resident_write import finish_job

    log = _as_log(puts)
    _check_block_size(block_size)
    if log.n == 0:
        raise ValueError("an SSTable needs at least one record (the reference fails in MetaBlock.to_bytes)")
    dev = _default_device if device is None else int(device)
    kin, ko, vin, vo = _log_arrays(log)
    job = _vp()
    rc = _native.lib().pbf_flush_begin(dev, _ptr(kin), _vp(ko.ctypes.data), _ptr(vin), _vp(vo.ctypes.data), log.n,
                                       block_size, ctypes.byref(job))
    if rc == _native.PBF_ERR_INVALID and "larger than block_size" in _native.lib().pbf_last_error().decode():
        raise ValueError("a record is larger than block_size (the reference would drop it, blocks.py:84-85)")
    _native.check(rc, "pbf_flush_begin")
    return finish_job(job, 1, fp_rate, dev)[0]


def flush_wal_resident(wal, block_size: int = BLOCK_SIZE, fp_rate: float = 0.001, device=None):
    """``flush_wal`` without the way back: `wal` as there, then ``flush_log_resident``."""
    return flush_log_resident(_wal_log(wal), block_size, fp_rate, device)
