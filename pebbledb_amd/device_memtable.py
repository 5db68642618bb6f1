"""The memtable on the device: ``MemTable`` (reference src/memtable.py) as one resident sorted
run, in front of the tables in ``LsmStorage.get`` (src/lsm_storage.py:153-162) and
``LsmStorage.scan`` (:184-190).

``put`` buffers on the host in put order (as ``BloomFilter.add`` buffers keys); the next read,
flush or ``sync()`` hands the buffered log to ``pbf_mt_apply``, which sorts it on the device
(``sort_log``'s chain) and merges it with the resident run, the new batch winning every shared
key (the tree replaces the data of a key it holds, src/red_black_tree.py:118-120).  Reads search
the run on the device (csrc/memtable_read_kernels.hpp).

Semantics kept from the reference: the last put of a key wins; ``get`` returns the value or None,
and a stored empty value is ``b""`` (``LsmStorage.get`` tests ``is not None``: a hit); there are no
tombstones.  ``approximate_size`` is the reference's: the sum of ``Record.size`` of every put,
re-puts included (memtable.py:68-72).

Divergence (an input the reference mishandles): ``MemTable.scan(lower, upper)`` walks the tree
with ``Node.in_order_traversal`` (src/red_black_tree.py:56-69), which leaves a whole subtree as
soon as its root lies outside the bounds and so drops in-range keys of the other child (DESIGN.md
§3: 899 of 900 random bounded scans over 300 keys came back short).  ``scan`` here has the
semantics of ``DeviceSSTable.scan``: ``lower <= key <= upper`` inclusive, ``lower > upper`` empty,
``upper == ""`` open, bounds compared as UTF-8 bytes.  With this rule a store's scan does not
change when a memtable is flushed.

A non-ASCII key is refused at ``put`` with ``flush_log``'s wording; probe keys and scan bounds may
be any ``str``.
"""
from __future__ import annotations

import ctypes
import threading
from typing import Optional

import numpy as np

from . import _native
from .keys import PackedKeys, PackedRecords
from .memtable import _as_log, _log_arrays, _ptr, _wal_log
from .sstable_data import BLOCK_SIZE, _check_block_size, build_sstable

_vp = ctypes.c_void_p
_u64 = ctypes.c_uint64
MAX_MEMTABLES = 16  # PBF_MT_MAX_PER_CALL

_NON_ASCII = ("a put log with a non-ASCII key cannot be flushed: the reference writes key_size in "
              "characters (record.py:25) and cannot read such a record back")


def _mt_handles(memtables):
    """The handles of the memtables of one call (buffered puts applied first)."""
    memtables = list(memtables)
    if len(memtables) > MAX_MEMTABLES:
        raise ValueError(f"a call takes at most {MAX_MEMTABLES} memtables, got {len(memtables)}")
    devs = {m.device for m in memtables}
    if len(devs) > 1:
        raise ValueError(f"all memtables of one call must share a device, got devices {sorted(devs)}")
    for m in memtables:
        m.sync()
    return (_vp * max(len(memtables), 1))(*[m._handle().value for m in memtables])


def _pack(keys) -> PackedKeys:
    return keys if isinstance(keys, PackedKeys) else PackedKeys.from_strs(list(keys))


def mt_lookup(memtables, keys):
    """``pbf_mt_get`` over host memory: (src int32[n], val_off uint64[n], val_len int32[n],
    miss_mask uint8[ceil(n/8)])."""
    pk = _pack(keys)
    n = pk.n
    src = np.full(n, -1, dtype=np.int32)
    vo = np.zeros(n, dtype=np.uint64)
    vl = np.full(n, -1, dtype=np.int32)
    miss = np.zeros((n + 7) // 8, dtype=np.uint8)
    hs = _mt_handles(memtables)
    if n:
        kd = pk.data if pk.data.size else np.zeros(1, np.uint8)
        rc = _native.lib().pbf_mt_get(hs, len(memtables), _vp(kd.ctypes.data),
                                      None if pk.offsets is None else _vp(pk.offsets.ctypes.data), pk.key_len, n, 0,
                                      None, _vp(src.ctypes.data), _vp(vo.ctypes.data), _vp(vl.ctypes.data),
                                      _vp(miss.ctypes.data))
        _native.check(rc, "pbf_mt_get")
    return src, vo, vl, miss


def mt_gather(memtables, tables, where, val_off, val_len):
    """``pbf_mt_gather`` over host memory: (values uint8[], value_offsets uint64[n+1])."""
    from .sstable_read import _handles

    where = np.ascontiguousarray(where, dtype=np.int32)
    val_off = np.ascontiguousarray(val_off, dtype=np.uint64)
    val_len = np.ascontiguousarray(val_len, dtype=np.int32)
    n = where.size
    total = int(np.clip(val_len, 0, None).sum(dtype=np.int64))
    out = np.empty(total, dtype=np.uint8)
    offs = np.zeros(n + 1, dtype=np.uint64)
    tables = list(tables)
    rc = _native.lib().pbf_mt_gather(_mt_handles(memtables), len(memtables), _handles(tables) if tables else None,
                                     len(tables), _ptr(where), _ptr(val_off), _ptr(val_len), n, _ptr(out), total,
                                     _vp(offs.ctypes.data), 0, None)
    _native.check(rc, "pbf_mt_gather")
    return out, offs


class DeviceMemTable:
    """``MemTable`` with its records resident on one device (see the module docstring)."""

    def __init__(self, device=None):
        from .bloom_filter import _default_device

        self.device = _default_device if device is None else int(device)
        self._h: Optional[ctypes.c_void_p] = None  # created by the first call that needs the device
        self._closed = False
        self._lock = threading.Lock()  # the put buffer's
        self._buf: list = []           # (key, value) in put order, not yet applied
        self.approximate_size = 0

    @classmethod
    def from_wal(cls, wal, device=None) -> "DeviceMemTable":
        """``MemTable.create_from_wal`` (memtable.py:29-53): `wal` is the path of a WAL file or its
        bytes."""
        self = cls(device)
        self.put_many(_wal_log(wal))
        return self

    # ------------------------------------------------------------------ writes
    def put(self, key: str, value: bytes) -> None:
        """``MemTable.put`` (memtable.py:64-72) without the WAL write, which stays with the caller."""
        if not isinstance(key, str) or not isinstance(value, (bytes, bytearray, memoryview)):
            raise TypeError("put takes a str key and a bytes value")
        if not key.isascii():
            raise ValueError(_NON_ASCII)
        value = bytes(value)
        with self._lock:
            if self._closed:
                raise ValueError("the memtable is closed")
            self._buf.append((key, value))
            self.approximate_size += 8 + len(key) + len(value)

    def put_many(self, keys, values=None) -> None:
        """``put`` for a batch in put order: `keys` and `values` of equal length, or (values None)
        a ``PackedRecords`` / an iterable of (key, value) pairs."""
        if values is not None:
            keys, values = list(keys), list(values)
            if len(keys) != len(values):
                raise ValueError("keys and values must have the same length")
            log = PackedRecords.from_iter(zip(keys, values))
        else:
            log = keys if isinstance(keys, PackedRecords) else PackedRecords.from_iter(keys)
        log = _as_log(log)
        with self._lock:
            self._handle()
            self._flush_buffer_locked()
            self.approximate_size += self._apply(log)

    def _apply(self, log: PackedRecords) -> int:
        """Hands a put log to the device; returns the sum of its records' sizes (Record.size)."""
        if log.n == 0:
            return 0
        kin, ko, vin, vo = _log_arrays(log)
        rc = _native.lib().pbf_mt_apply(self._h, _ptr(kin), _vp(ko.ctypes.data), _ptr(vin), _vp(vo.ctypes.data), log.n)
        _native.check(rc, "pbf_mt_apply")
        return 8 * log.n + int(ko[-1]) + int(vo[-1])

    def _flush_buffer_locked(self) -> None:
        if self._buf:
            buf, self._buf = self._buf, []
            self._apply(PackedRecords.from_iter(buf))

    def sync(self) -> None:
        """Applies the buffered puts to the resident run."""
        with self._lock:
            self._handle()
            self._flush_buffer_locked()

    # ------------------------------------------------------------------ reads
    def _handle(self):
        if self._closed:
            raise ValueError("the memtable is closed")
        if self._h is None:
            h = _vp()
            _native.check(_native.lib().pbf_mt_create(self.device, ctypes.byref(h)), "pbf_mt_create")
            self._h = h
        return self._h

    def _info(self):
        self.sync()
        n, kb, vb = _u64(), _u64(), _u64()
        _native.check(_native.lib().pbf_mt_info(self._h, ctypes.byref(n), ctypes.byref(kb), ctypes.byref(vb)),
                      "pbf_mt_info")
        return n.value, kb.value, vb.value

    def __len__(self) -> int:
        """The distinct keys held."""
        return self._info()[0]

    def get_many(self, keys) -> list:
        """[MemTable.get(key) for key in keys]: bytes (``b""`` for a stored empty value), or None."""
        pk = _pack(keys)
        src, vo, vl, _ = mt_lookup([self], pk)
        vals, offs = mt_gather([self], [], np.where(src >= 0, -2 - src, -1), vo, vl)
        raw = vals.tobytes()
        return [raw[int(offs[i]):int(offs[i + 1])] if src[i] >= 0 else None for i in range(pk.n)]

    def get(self, key: str) -> Optional[bytes]:
        """``MemTable.get`` (memtable.py:74-79)."""
        return self.get_many([key])[0]

    def records(self) -> PackedRecords:
        """``MemTableIterator(memtable)`` as a packed run: ``sort_log`` of every put so far."""
        n, kb, vb = self._info()
        keys, values = np.empty(kb, dtype=np.uint8), np.empty(vb, dtype=np.uint8)
        ko, vo = np.empty(n + 1, dtype=np.uint64), np.empty(n + 1, dtype=np.uint64)
        rc = _native.lib().pbf_mt_read(self._h, _ptr(keys), kb, _vp(ko.ctypes.data), _ptr(values), vb,
                                       _vp(vo.ctypes.data), n + 1)
        _native.check(rc, "pbf_mt_read")
        return PackedRecords(PackedKeys(keys, n, offsets=ko), values, vo, ascii=True)

    def scan(self, lower: str, upper: str) -> PackedRecords:
        """The records with ``lower <= key <= upper`` (``upper == ""``: no upper bound) as a packed
        run; see the module docstring for the divergence from the reference's ``MemTable.scan``."""
        from .lsm_scan import scan_ranges

        return scan_ranges([], [(lower, upper)], memtables=[self])[0]

    # ------------------------------------------------------------------ flush
    def flush_resident(self, block_size: int = BLOCK_SIZE, fp_rate: float = 0.001):
        """``_do_flush`` on the device (``flush_log_resident`` of every put so far, without the
        upload and the sort): the flushed table as an open ``DeviceSSTable``.  The memtable stays
        as it is."""
        from .resident_write import finish_job

        _check_block_size(block_size)
        if self._info()[0] == 0:
            raise ValueError("an SSTable needs at least one record (the reference fails in MetaBlock.to_bytes)")
        job = _vp()
        rc = _native.lib().pbf_mt_flush_begin(self._h, block_size, ctypes.byref(job))
        if rc == _native.PBF_ERR_INVALID and "larger than block_size" in _native.lib().pbf_last_error().decode():
            raise ValueError("a record is larger than block_size (the reference would drop it, blocks.py:84-85)")
        _native.check(rc, "pbf_mt_flush_begin")
        return finish_job(job, 1, fp_rate, self.device)[0]

    def flush(self, block_size: int = BLOCK_SIZE, fp_rate: float = 0.001):
        """What ``flush_log`` of every put so far returns (file bytes, meta blocks, filter)."""
        return build_sstable(self.records(), None, block_size, fp_rate, self.device)

    # ------------------------------------------------------------------ lifetime
    def close(self) -> None:
        """Frees the resident run (waits for reads in flight); every later call raises."""
        with self._lock:
            h, self._h = self._h, None
            self._closed = True
            self._buf = []
        if h is not None and _native._lib is not None:
            _native._lib.pbf_mt_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
