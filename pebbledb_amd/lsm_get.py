"""The filter stage of ``LsmStorage.get`` over a batch of keys (reference
src/lsm_storage.py:153-179).

For one key the reference walks the SSTables in a fixed order and reads (``SSTable.get``) the
first ones its checks let through:

* L0, newest first (``sstables_level0``): ``bloom_filter.may_contain(key)`` (:164-169);
* every level L>=1, each SSTable in list order: ``first_key <= key <= last_key`` (:173),
  then ``may_contain(key)`` (:175).

``candidate_masks`` computes both checks for a whole batch on the device: the L0 filters and
the range-qualified level filters are probed with ``may_contain_multi`` (one shared pipeline
per SSTable size class), and the level key-range check is ``pbf_key_range_mask`` (bytewise
compare of the UTF-8 keys = Python ``str`` order).  The result is one LSB-first mask per
SSTable, numbered L0 first then level by level (``shard.candidate_order``'s numbering), whose
set bits are exactly the (key, SSTable) pairs the reference would go on to read, in the
reference's order (``candidate_lists``).  A level SSTable whose range holds no key of the batch
is never probed, as the reference never probes it.

``candidates_one`` is the per-key form (one ``get``): the range checks are Python's own ``str``
comparison on the host, and every L0 filter plus every in-range level filter is tested in ONE
launch (``pbf_may_contain_set``), whatever the filters' sizes — instead of one ``may_contain``
launch per SSTable.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple, Sequence

import numpy as np

from . import _native
from . import bloom_filter as _bfm
from .bloom_filter import (BloomFilter, _default_device, may_contain_multi, may_contain_set_bits,
                           probe_multi_device)
from .keys import PackedKeys


class LevelTable(NamedTuple):
    """An L>=1 SSTable as LsmStorage.get sees it (sstable.first_key / last_key / bloom_filter)."""
    first_key: str
    last_key: str
    bloom_filter: BloomFilter


def _pack(keys) -> PackedKeys:
    return keys if isinstance(keys, PackedKeys) else PackedKeys.from_strs(list(keys))


def key_range_masks(keys, bounds: Sequence[tuple[str, str]], device: int | None = None) -> np.ndarray:
    """uint8 [len(bounds), ceil(n/8)]: bit i of row t = ``first_t <= key_i <= last_t``
    (lsm_storage.py:173), computed by ``pbf_key_range_mask`` on the device."""
    pk = _pack(keys)
    nb = (pk.n + 7) // 8
    out = np.zeros((len(bounds), nb), dtype=np.uint8)
    if pk.n == 0 or not bounds:
        return out
    enc = [s.encode("utf-8") for pair in bounds for s in pair]
    lens = np.fromiter(map(len, enc), dtype=np.int64, count=len(enc))
    boffs = np.zeros(len(enc) + 1, dtype=np.uint64)
    np.cumsum(lens, out=boffs[1:])
    bbytes = np.frombuffer(b"".join(enc) or b"\0", dtype=np.uint8)
    keys_arr = pk.data if pk.data.size else np.zeros(1, np.uint8)
    vp = ctypes.c_void_p
    dev = _default_device if device is None else int(device)
    rc = _native.lib().pbf_key_range_mask(dev, None, vp(keys_arr.ctypes.data),
                                          None if pk.offsets is None else vp(pk.offsets.ctypes.data), pk.key_len,
                                          pk.n, vp(bbytes.ctypes.data), vp(boffs.ctypes.data), len(bounds),
                                          vp(out.ctypes.data), 0)
    _native.check(rc, "pbf_key_range_mask")
    return out


def candidate_masks(keys, level0: Sequence[BloomFilter], levels: Sequence[Sequence[LevelTable]]) -> np.ndarray:
    """uint8 [T, ceil(n/8)], T = len(level0) + sum(len(level)): row t's bit i is set iff
    LsmStorage.get(key_i) would read SSTable t if no earlier SSTable held the key
    (lsm_storage.py:164-179).  Rows: L0 in the given (newest-first) order, then each level's
    SSTables in list order."""
    pk = _pack(keys)
    nb = (pk.n + 7) // 8
    flat = [t for lvl in levels for t in lvl]
    level0 = [getattr(f, "bloom_filter", f) for f in level0]  # a DeviceSSTable stands for its filter
    out = np.zeros((len(level0) + len(flat), nb), dtype=np.uint8)
    if pk.n == 0:
        return out
    if level0:
        out[:len(level0)] = _probe_rows(level0, pk)
    if flat:
        rng = key_range_masks(pk, [(t.first_key, t.last_key) for t in flat],
                              device=flat[0].bloom_filter.device)
        live = [j for j in range(len(flat)) if rng[j].any()]  # tables no key of the batch reaches
        if live:
            hits = _probe_rows([flat[j].bloom_filter for j in live], pk)
            for r, j in enumerate(live):
                out[len(level0) + j] = rng[j] & hits[r]
    return out


def _probe_rows(filters, pk: PackedKeys) -> np.ndarray:
    """``may_contain_multi`` row per entry of `filters`; a filter object that stands behind
    several tables (``pbf_probe_multi`` takes each filter once) is probed once and its row shared."""
    first = {}
    slot = [first.setdefault(id(f), len(first)) for f in filters]
    if len(first) == len(filters):
        return may_contain_multi(filters, pk)
    distinct = [None] * len(first)
    for f, s in zip(filters, slot):
        distinct[s] = f
    return may_contain_multi(distinct, pk)[slot]


def candidate_lists(masks: np.ndarray, n: int) -> list[list[int]]:
    """Per key, the SSTable rows of ``candidate_masks`` in the reference's read order."""
    bits = np.unpackbits(masks, axis=1, bitorder="little")[:, :n].astype(bool)
    return [[int(t) for t in np.flatnonzero(bits[:, i])] for i in range(n)]


def candidates_one(key: str, level0: Sequence[BloomFilter], levels: Sequence[Sequence[LevelTable]]) -> list[int]:
    """The SSTables ``LsmStorage.get(key)`` would read if none held the key, in its order
    (lsm_storage.py:164-179), numbered as ``candidate_masks`` rows: L0 filters (newest first)
    and the level filters whose ``first_key <= key <= last_key`` (:173) are tested together in
    one ``pbf_may_contain_set`` launch.  The whole stage runs in C (``_pebblefast.candidates_one``:
    the range checks, the handles and the call, ~3 us less per get than this loop); it hands back
    None when this path must take the call (buffered adds, a non-str key, filters on several
    devices, more than 64 filters), which then raises what the reference raises."""
    r = (_bfm._FAST or _bfm._fast()).candidates_one(key, level0, levels)
    if r is not None:
        return r
    n0 = len(level0)
    if n0 and not isinstance(key, str):
        # the reference probes L0 before any level's range check (:164-165): its bloom check's
        # AttributeError (key.encode) comes before the TypeError of `str <= key` (:173)
        may_contain_set_bits(list(level0), key)
    in_range, tested = [], list(level0)
    j = n0
    for lvl in levels:
        for t in lvl:
            if t.first_key <= key <= t.last_key:
                in_range.append(j)
                tested.append(t.bloom_filter)
            j += 1
    if not tested:
        return []
    bits = may_contain_set_bits(tested, key)
    out = list(_set_bits(bits & ((1 << n0) - 1)))
    if in_range:
        out += [in_range[r] for r in _set_bits(bits >> n0)]
    return out


_SET_BITS: dict = {}


def _set_bits(b: int) -> tuple:
    """The indices of b's set bits, ascending (memoised: a get's hit pattern over its L0 and
    in-range tables repeats)."""
    r = _SET_BITS.get(b)
    if r is None:
        r = tuple(i for i in range(b.bit_length()) if b >> i & 1)
        if len(_SET_BITS) < 1 << 16:
            _SET_BITS[b] = r
    return r


# ---------------------------------------------------------------------------- get: keys in, values out
def _walk_device(keys_ptr: int, offsets_ptr: int, key_len: int, n: int, level0, flat, device: int, timings=None,
                 memtables=()):
    """The whole batched get on device memory (torch tensors hold the buffers): the filter and
    key-range stage in their device-pointer forms (``probe_multi_device``,
    ``pbf_key_range_mask`` with on_device=1), so the candidate masks never leave the GPU, then
    ``pbf_sst_get`` and ``pbf_sst_gather``, all ordered on torch's current stream.  Returns device
    tensors (table int32[n], values uint8[total], value_offsets int64[n+1], val_len int32[n]).
    `timings`: a dict that receives HIP-event times of the three stages in ms.
    With `memtables` the memtable stage (``pbf_mt_get``) runs first on the same stream; its miss
    mask is ANDed into every table's candidate mask, so a key a memtable answered is searched in
    no table, and ``pbf_mt_gather`` packs the values of both kinds of hit (timings: memtable_ms)."""
    import torch

    from .sstable_read import _handles

    tables = list(level0) + list(flat)
    memtables = list(memtables)
    hs = _handles(tables) if tables else None
    mts = None
    if memtables:
        from .device_memtable import _mt_handles
        mts = _mt_handles(memtables)
    n0, T, nb = len(level0), len(tables), (n + 7) // 8
    dev = torch.device("cuda", device)
    vp = ctypes.c_void_p
    L = _native.lib()
    with torch.cuda.device(dev):
        cur = torch.cuda.current_stream(dev)
        sp = cur.cuda_stream

        def mark():
            e = torch.cuda.Event(enable_timing=True)
            e.record(cur)
            return e

        masks = torch.zeros((T, nb), dtype=torch.uint8, device=dev)
        em = mark()
        if mts is not None:  # lsm_storage.py:154-162: the memtables answer first
            msrc = torch.empty(n, dtype=torch.int32, device=dev)
            mvo = torch.empty(n, dtype=torch.int64, device=dev)
            mvl = torch.empty(n, dtype=torch.int32, device=dev)
            miss = torch.empty(nb, dtype=torch.uint8, device=dev)
            rc = L.pbf_mt_get(mts, len(memtables), vp(keys_ptr), vp(offsets_ptr or None), key_len, n, 1, vp(sp or None),
                              vp(msrc.data_ptr()), vp(mvo.data_ptr()), vp(mvl.data_ptr()), vp(miss.data_ptr()))
            _native.check(rc, "pbf_mt_get")
        e0 = mark()
        if level0:
            f0 = [t.bloom_filter for t in level0]
            f0[0].wait_stream(sp)
            probe_multi_device(f0, keys_ptr, n, [masks[i].data_ptr() for i in range(n0)], key_len, offsets_ptr)
            f0[0].signal_stream(sp)
        if flat:
            enc = [s.encode("utf-8") for t in flat for s in (t.first_key, t.last_key)]
            boffs = np.zeros(len(enc) + 1, dtype=np.int64)
            np.cumsum(np.fromiter(map(len, enc), dtype=np.int64, count=len(enc)), out=boffs[1:])
            bbytes = torch.from_numpy(np.frombuffer(b"".join(enc) or b"\0", dtype=np.uint8).copy()).to(dev)
            boffs_d = torch.from_numpy(boffs).to(dev)
            rng = torch.empty((len(flat), nb), dtype=torch.uint8, device=dev)
            rc = L.pbf_key_range_mask(device, vp(sp or None), vp(keys_ptr), vp(offsets_ptr or None), key_len, n,
                                      vp(bbytes.data_ptr()), vp(boffs_d.data_ptr()), len(flat), vp(rng.data_ptr()), 1)
            _native.check(rc, "pbf_key_range_mask")
            fl = [t.bloom_filter for t in flat]
            fl[0].wait_stream(sp)
            probe_multi_device(fl, keys_ptr, n, [masks[n0 + j].data_ptr() for j in range(len(flat))], key_len,
                               offsets_ptr)
            fl[0].signal_stream(sp)
            masks[n0:] &= rng  # lsm_storage.py:173-175: in range, then may_contain
        if mts is not None and T:
            masks &= miss  # a key a memtable holds is searched in no table
        e1 = mark()
        if T:
            table = torch.empty(n, dtype=torch.int32, device=dev)
            val_off = torch.empty(n, dtype=torch.int64, device=dev)
            val_len = torch.empty(n, dtype=torch.int32, device=dev)
            mp = (vp * T)(*[masks[t].data_ptr() for t in range(T)])
            rc = L.pbf_sst_get(hs, T, vp(keys_ptr), vp(offsets_ptr or None), key_len, n, mp, 1, vp(sp or None),
                               vp(table.data_ptr()), vp(val_off.data_ptr()), vp(val_len.data_ptr()))
            _native.check(rc, "pbf_sst_get")
        if mts is not None:  # table[i] = -2 - m for a hit in memtable m
            hit = msrc >= 0
            table = torch.where(hit, -2 - msrc, table) if T else torch.where(hit, -2 - msrc, msrc)
            val_off = torch.where(hit, mvo, val_off) if T else mvo
            val_len = torch.where(hit, mvl, val_len) if T else mvl
        e2 = mark()
        total = int(val_len.clamp(min=0).sum(dtype=torch.int64).item())
        offs = torch.empty(n + 1, dtype=torch.int64, device=dev)
        vals = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
        e3 = mark()
        if mts is not None:
            rc = L.pbf_mt_gather(mts, len(memtables), hs, T, vp(table.data_ptr()), vp(val_off.data_ptr()),
                                 vp(val_len.data_ptr()), n, vp(vals.data_ptr()) if total else None, total,
                                 vp(offs.data_ptr()), 1, vp(sp or None))
            _native.check(rc, "pbf_mt_gather")
        else:
            rc = L.pbf_sst_gather(hs, T, vp(table.data_ptr()), vp(val_off.data_ptr()), vp(val_len.data_ptr()), n,
                                  vp(vals.data_ptr()) if total else None, total, vp(offs.data_ptr()), 1, vp(sp or None))
            _native.check(rc, "pbf_sst_gather")
        e4 = mark()
        cur.synchronize()
        if timings is not None:
            timings.update(filter_ms=e0.elapsed_time(e1), walk_ms=e1.elapsed_time(e2), gather_ms=e3.elapsed_time(e4))
            if mts is not None:
                timings.update(memtable_ms=em.elapsed_time(e0))
    return table, vals[:total], offs, val_len


def get_batch(keys, level0, levels, memtables=()):
    """``LsmStorage.get`` for a batch of keys (lsm_storage.py:153-179), keys in, values out: (table
    int32[n], values uint8[], value_offsets uint64[n+1]).  `memtables` = [active, *immutables]
    (``DeviceMemTable``s, at most 16, on the tables' device) are searched first, in that order;
    ``memtables=()`` is the get with empty memtables.  table[i] is ``-2 - m`` when memtable m
    answered key i (a stored empty value is an answer), otherwise the row
    (``candidate_masks``' numbering: L0 newest first, then level by level) of the SSTable whose
    value the reference returns for key i, -1 when it returns None; value i =
    values[value_offsets[i]:value_offsets[i+1]] (empty when absent, and for a stored empty value,
    which the reference returns as ``b""``).  `level0` and each level hold ``DeviceSSTable``s on
    one device.  The keys go to the device once; the candidate masks are computed and consumed
    there (``_walk_device``)."""
    import torch

    pk = _pack(keys)
    level0 = list(level0)
    flat = [t for lvl in levels for t in lvl]
    tables = level0 + flat
    memtables = list(memtables)
    n = pk.n
    if n == 0 or not (tables or memtables):
        return np.full(n, -1, dtype=np.int32), np.zeros(0, dtype=np.uint8), np.zeros(n + 1, dtype=np.uint64)
    devs = {t.device for t in tables}
    if len(devs) > 1:
        raise ValueError(f"all tables of one call must share a device, got devices {sorted(devs)}")
    if len(memtables) > 16:  # PBF_MT_MAX_PER_CALL
        raise ValueError(f"a call takes at most 16 memtables, got {len(memtables)}")
    if len(devs | {m.device for m in memtables}) > 1:
        raise ValueError("the memtables and tables of one call must share a device")
    device = (tables or memtables)[0].device
    dev = torch.device("cuda", device)
    def upload(a):  # (torch wants a writable array: packed keys may view an immutable bytes object)
        return torch.from_numpy(a if a.flags.writeable else a.copy()).to(dev)

    kd = upload(pk.data if pk.data.size else np.zeros(1, np.uint8))
    od = None if pk.offsets is None else upload(pk.offsets.view(np.int64))
    table, vals, offs, _ = _walk_device(kd.data_ptr(), 0 if od is None else od.data_ptr(), pk.key_len, n, level0, flat,
                                        device, memtables=memtables)
    return table.cpu().numpy(), vals.cpu().numpy(), offs.cpu().numpy().view(np.uint64)


def get_many(keys, level0, levels, memtables=()) -> list:
    """[LsmStorage.get(key) for key in keys] (`memtables` as in ``get_batch``): bytes, or None."""
    table, vals, offs = get_batch(keys, level0, levels, memtables)
    raw = vals.tobytes()
    return [raw[int(offs[i]):int(offs[i + 1])] if table[i] != -1 else None for i in range(len(table))]
