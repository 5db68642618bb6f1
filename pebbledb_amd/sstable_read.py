"""SSTable point lookup on the device: ``SSTable.build_from_path`` / ``SSTable.get`` (reference
src/sstable.py:150-206) for batches of keys, over tables whose data sections are resident in HBM.

``DeviceSSTable.from_bytes`` parses the trailer and the meta blocks on the host
(sstable.py:89-113, blocks.py:142-151), loads the bloom filter (``BloomFilter.from_bytes``) and
opens the data section as a resident table (``pbf_sst_open``): one copy to the device, where
every block is validated (csrc/sstable_read_kernels.hpp ``k_sst_validate``) and a block index is
written.  ``get_many`` then answers a batch with ``pbf_sst_get`` (one lane per key: a binary
search over the block index, another over the block's u16 offsets) and ``pbf_sst_gather`` (an
exclusive scan of the value lengths, then one packed copy of the found values).

The reference's lookup is linear: the first meta block whose ``last_key >= key``, then
``first_key <= key``, then the first record of the block whose key equals the probe.  For
strictly ascending keys the binary searches give exactly that answer; flush and compaction only
write such tables (memtable and merging iterators).  A stored empty value is found
(``val_len == 0``, the reference returns ``b""`` because it tests ``is not None``).

Divergences (inputs the reference mishandles): a table that is not strictly ascending, or whose
record sizes do not match their extents, raises ValueError at open.  The second rule refuses every
table that stores a non-ASCII key: the reference writes ``key_size = len(str)`` in characters
(record.py:25) and reads it back as a byte count (record.py:77-79), so it cannot read such a table
itself (``get`` of the stored key returns None, ``get`` of a shorter key returns garbage).  Probe
keys may be any ``str``; a non-ASCII probe key is simply absent.

Tables stay resident until ``close()`` (or garbage collection): there is no block cache and no
eviction.
"""
from __future__ import annotations

import ctypes
import struct
from typing import Optional, Sequence

import numpy as np

from . import _native
from .bloom_filter import BloomFilter, _default_device
from .keys import PackedKeys
from .sstable_bloom import bloom_section_bounds

_vp = ctypes.c_void_p


def parse_meta_blocks(meta: bytes) -> list[tuple[str, str, int]]:
    """MetaBlock.from_bytes over the meta section (sstable.py:103-108, blocks.py:142-151):
    [(first_key, last_key, offset)].  A section that does not parse raises ValueError."""
    out, o, n = [], 0, len(meta)
    try:
        while o < n:
            fs, = struct.unpack_from("H", meta, o)
            first = meta[o + 2:o + 2 + fs]
            ls, = struct.unpack_from("H", meta, o + 2 + fs)
            last = meta[o + 4 + fs:o + 4 + fs + ls]
            off, = struct.unpack_from("i", meta, o + 4 + fs + ls)
            if len(first) != fs or len(last) != ls:
                raise ValueError("meta block runs past the meta section")
            out.append((first.decode("utf-8"), last.decode("utf-8"), off))
            o += 8 + fs + ls
    except (struct.error, UnicodeDecodeError) as e:
        raise ValueError(f"meta blocks do not parse: {e}") from None
    return out


def _as_u8(buf) -> np.ndarray:
    if isinstance(buf, np.ndarray):
        return np.ascontiguousarray(buf, dtype=np.uint8).reshape(-1)
    return np.frombuffer(buf, dtype=np.uint8)


def _pack(keys) -> PackedKeys:
    return keys if isinstance(keys, PackedKeys) else PackedKeys.from_strs(list(keys))


def _handles(tables):
    devs = {t.device for t in tables}
    if len(devs) > 1:
        raise ValueError(f"all tables of one call must share a device, got devices {sorted(devs)}")
    for t in tables:
        if t._h is None:
            raise ValueError("the SSTable is closed")
    return (_vp * len(tables))(*[t._h.value for t in tables])


def lookup(tables: Sequence["DeviceSSTable"], keys, masks=None):
    """``pbf_sst_get`` over host memory: (table int32[n], val_off uint64[n], val_len int32[n]).
    `masks`: None, or one entry per table — None (every key) or a packed LSB-first uint8 mask."""
    pk = _pack(keys)
    n = pk.n
    table = np.full(n, -1, dtype=np.int32)
    val_off = np.zeros(n, dtype=np.uint64)
    val_len = np.full(n, -1, dtype=np.int32)
    hs = _handles(tables)
    if n == 0 or not tables:
        return table, val_off, val_len
    nb = (n + 7) // 8
    mp = None
    if masks is not None:
        if len(masks) != len(tables):
            raise ValueError("one mask (or None) per table")
        keep = [None if m is None else np.ascontiguousarray(m, dtype=np.uint8).reshape(-1) for m in masks]
        for m in keep:
            if m is not None and m.size != nb:
                raise ValueError(f"a mask holds ceil(n/8) = {nb} bytes")
        mp = (_vp * len(tables))(*[None if m is None else m.ctypes.data for m in keep])
    kd = pk.data if pk.data.size else np.zeros(1, np.uint8)
    rc = _native.lib().pbf_sst_get(hs, len(tables), _vp(kd.ctypes.data),
                                   None if pk.offsets is None else _vp(pk.offsets.ctypes.data), pk.key_len, n, mp, 0,
                                   None, _vp(table.ctypes.data), _vp(val_off.ctypes.data), _vp(val_len.ctypes.data))
    _native.check(rc, "pbf_sst_get")
    return table, val_off, val_len


def gather(tables: Sequence["DeviceSSTable"], table, val_off, val_len):
    """``pbf_sst_gather`` over host memory: (values uint8[], value_offsets uint64[n+1])."""
    n = len(val_len)
    offs = np.zeros(n + 1, dtype=np.uint64)
    total = int(np.maximum(val_len, 0).sum(dtype=np.int64)) if n else 0
    out = np.empty(total, dtype=np.uint8)
    if n == 0 or not tables:
        return out, offs
    hs = _handles(tables)
    table = np.ascontiguousarray(table, dtype=np.int32)
    val_off = np.ascontiguousarray(val_off, dtype=np.uint64)
    val_len = np.ascontiguousarray(val_len, dtype=np.int32)
    rc = _native.lib().pbf_sst_gather(hs, len(tables), _vp(table.ctypes.data), _vp(val_off.ctypes.data),
                                      _vp(val_len.ctypes.data), n, _vp(out.ctypes.data) if total else None, total,
                                      _vp(offs.ctypes.data), 0, None)
    _native.check(rc, "pbf_sst_gather")
    return out, offs


class DeviceSSTable:
    """An SSTable whose data section is resident on the device (see the module docstring).  Has
    the attributes LsmStorage.get reads (``first_key``, ``last_key``, ``bloom_filter``), so it
    stands where ``lsm_get.LevelTable`` stands; ``lsm_get.candidate_masks`` also takes it in
    level 0, where a bare filter stands."""

    def __init__(self):
        raise TypeError("use DeviceSSTable.from_bytes / from_path")

    @classmethod
    def from_path(cls, path: str, device: Optional[int] = None) -> "DeviceSSTable":
        """SSTable.build_from_path (sstable.py:192-206)."""
        with open(path, "rb") as f:
            return cls.from_bytes(f.read(), device=device)

    @classmethod
    def from_bytes(cls, file_bytes, device: Optional[int] = None) -> "DeviceSSTable":
        """SSTableEncoding.from_bytes (sstable.py:88-113) of a whole file buffer (bytes,
        bytearray, memoryview or a uint8 array such as ``build_sstable`` returns)."""
        buf = _as_u8(file_bytes)
        meta_offset, bloom_offset, end = bloom_section_bounds(buf)
        metas = parse_meta_blocks(buf[meta_offset:bloom_offset].tobytes())
        if not metas:
            raise ValueError("an SSTable needs at least one data block")
        offs = [m[2] for m in metas] + [meta_offset]
        if offs[0] != 0 or any(b < a for a, b in zip(offs, offs[1:])):
            raise ValueError("meta block offsets must ascend from 0 to the data section's end")
        self = object.__new__(cls)
        self._h = None
        self.device = _default_device if device is None else int(device)
        self.meta_blocks = metas
        self.meta_block_offset = meta_offset
        self.first_key, self.last_key = metas[0][0], metas[-1][1]
        self.bloom_filter = BloomFilter.from_bytes(memoryview(buf)[bloom_offset:end], device=self.device)
        block_off = np.asarray(offs, dtype=np.uint32)
        data = buf[:meta_offset]
        h = _vp()
        rc = _native.lib().pbf_sst_open(self.device, _vp(data.ctypes.data) if data.size else None, meta_offset,
                                        _vp(block_off.ctypes.data), len(metas), 0, ctypes.byref(h))
        _native.check(rc, "pbf_sst_open")
        self._h = h
        nb, nr, dl = ctypes.c_uint32(), ctypes.c_uint64(), ctypes.c_uint64()
        _native.check(_native.lib().pbf_sst_info(h, ctypes.byref(nb), ctypes.byref(nr), ctypes.byref(dl)), "pbf_sst_info")
        self.nblocks, self.nrecords, self.data_len = nb.value, nr.value, dl.value
        try:
            self._check_meta_keys(data)
        except ValueError:
            self.close()
            raise
        return self

    @classmethod
    def _from_handle(cls, handle, device: int, metas, bloom: BloomFilter, nblocks: int, nrecords: int,
                     data_len: int) -> "DeviceSSTable":
        """A table the device built in place (``resident_write``): the attributes ``from_bytes``
        sets, from what the job reported."""
        self = object.__new__(cls)
        self._h = handle
        self.device = device
        self.meta_blocks = metas
        self.meta_block_offset = data_len
        self.first_key, self.last_key = metas[0][0], metas[-1][1]
        self.bloom_filter = bloom
        self.nblocks, self.nrecords, self.data_len = nblocks, nrecords, data_len
        return self

    def to_bytes(self) -> np.ndarray:
        """The table's ``.sst`` file (SSTableEncoding.to_bytes, sstable.py:80-86) as a uint8 array:
        the data section copied from the device (``pbf_sst_read_data``), the meta blocks
        (MetaBlock.to_bytes, blocks.py:126-133), the bloom section and the trailer -- what
        ``build_sstable(s)`` returns for the same records, and for a table opened with
        ``from_bytes`` the bytes it was opened from."""
        from .sstable_bloom import TRAILER, sstable_size

        if self._h is None:
            raise ValueError("the SSTable is closed")
        meta = b"".join(struct.pack("H", len(first)) + first.encode("utf-8") + struct.pack("H", len(last)) +
                        last.encode("utf-8") + struct.pack("i", off) for first, last, off in self.meta_blocks)
        bloom = self.bloom_filter.to_bytes()  # bitmap and the k byte
        data_len = self.data_len
        if data_len + len(meta) > 0x7FFFFFFF:
            raise struct.error("'i' format requires -2147483648 <= number <= 2147483647")
        out = np.empty(sstable_size(data_len, len(meta), len(bloom) - 1), dtype=np.uint8)
        _native.check(_native.lib().pbf_sst_read_data(self._h, _vp(out.ctypes.data), data_len), "pbf_sst_read_data")
        bloom_off = data_len + len(meta)
        out[data_len:bloom_off] = np.frombuffer(meta, dtype=np.uint8)
        out[bloom_off:bloom_off + len(bloom)] = np.frombuffer(bloom, dtype=np.uint8)
        out[len(out) - TRAILER:] = np.frombuffer(struct.pack("ii", data_len, bloom_off), dtype=np.uint8)
        return out

    def write(self, path) -> None:
        """Writes ``to_bytes()`` to `path`."""
        with open(path, "wb") as f:
            f.write(self.to_bytes().data)

    def _check_meta_keys(self, data: np.ndarray) -> None:
        """Every meta block's first / last key is the key of the block's first / last record in
        the validated index (the lookup trusts the index; LsmStorage.get's range check trusts
        the meta blocks)."""
        idx = np.empty((self.nblocks, 4), dtype=np.uint32)
        _native.check(_native.lib().pbf_sst_block_index(self._h, _vp(idx.ctypes.data), self.nblocks),
                      "pbf_sst_block_index")
        raw = data.tobytes()

        def key_at(o: int) -> bytes:
            ks, = struct.unpack_from("i", raw, o)
            return raw[o + 4:o + 4 + ks]

        for b, (first, last, _) in enumerate(self.meta_blocks):
            if key_at(int(idx[b, 0])) != first.encode("utf-8") or key_at(int(idx[b, 1])) != last.encode("utf-8"):
                raise ValueError(f"meta block {b} does not name its data block's first and last keys")

    def close(self) -> None:
        """Frees the resident table (waits for lookups in flight)."""
        h, self._h = self._h, None
        if h is not None and _native._lib is not None:
            _native._lib.pbf_sst_close(h)

    def __del__(self):
        self.close()

    @property
    def handle(self):
        return self._h

    def get_many(self, keys, mask=None):
        """SSTable.get for a batch (`keys`: list[str] or PackedKeys): (found bool[n], values
        uint8[], value_offsets uint64[n+1]); value i = values[value_offsets[i]:value_offsets[i+1]]
        (empty for an absent key and for a stored empty value: ``found`` tells them apart).
        `mask`: bool[n] or a packed LSB-first uint8[ceil(n/8)]; a cleared key is not looked up."""
        pk = _pack(keys)
        if mask is not None:
            mask = np.asarray(mask)
            if mask.dtype == np.bool_:
                if mask.size != pk.n:
                    raise ValueError("a bool mask holds one entry per key")
                mask = np.packbits(mask, bitorder="little")
        table, val_off, val_len = lookup([self], pk, None if mask is None else [mask])
        values, offs = gather([self], table, val_off, val_len)
        return val_len >= 0, values, offs

    def get(self, key: str) -> Optional[bytes]:
        """SSTable.get (sstable.py:175-187)."""
        found, values, _ = self.get_many([key])
        return values.tobytes() if found[0] else None

    def records(self):
        """SSTableIterator(sstable) (src/iterators.py:110-141) as a PackedRecords: every record
        in key order (the one-table merge of ``compaction.merge_tables``)."""
        from .compaction import merge_tables
        return merge_tables([self])

    def scan(self, lower: str, upper: str):
        """SSTable.scan (sstable.py:189) as a PackedRecords: the records with ``lower <= key <=
        upper`` in key order; ``upper == ""`` means no upper bound, as in the reference
        (``lsm_scan.scan_tables`` over this one table)."""
        from .lsm_scan import scan_tables
        return scan_tables([self], lower, upper)

    def __repr__(self):
        return f"DeviceSSTable(nblocks={self.nblocks}, nrecords={self.nrecords}, device={self.device})"
