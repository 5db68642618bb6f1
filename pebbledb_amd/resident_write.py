"""The second phase of a resident write job (include/pebblebloom.h, "Resident write path"): after
``pbf_compact_begin`` / ``pbf_flush_begin`` have left the record run and its plan on the device,
size every output's filter from its own record count, let ``pbf_job_finish`` encode, build,
gather and validate on the device, and wrap the new handles as ``DeviceSSTable``s.

What stays on the host, and why: the filter sizing (the reference's float expression,
bloom_filter.py:109-114, with Python's ``round``: ``sstable_data.filter_sizing``) and the meta
blocks (``MetaBlock.to_bytes`` needs each block's first and last key and offset: a few bytes per
64 KiB block, which ``pbf_job_finish`` hands back).  The run itself never leaves the device; a
file is produced only when a caller asks (``DeviceSSTable.to_bytes`` / ``write``).
"""
from __future__ import annotations

import ctypes
import struct

import numpy as np

from . import _native
from .bloom_filter import BloomFilter
from .sstable_data import filter_sizing
from .sstable_read import DeviceSSTable

_vp = ctypes.c_void_p
_u64 = ctypes.c_uint64
JOB_STAGES = ("run", "plan", "encode", "filters", "validate")


def finish_job(job, ntables: int, fp_rate: float, device: int) -> list:
    """The job's outputs as ``DeviceSSTable``s, in the order ``_compact`` returns them.  The job
    is consumed: finished, or aborted when an output cannot be sized."""
    lib = _native.lib()
    try:
        infos, filters = [], []
        nr, nb, dl, kb = _u64(), _u64(), _u64(), _u64()
        for t in range(ntables):
            _native.check(lib.pbf_job_table_info(job, t, ctypes.byref(nr), ctypes.byref(nb), ctypes.byref(dl),
                                                 ctypes.byref(kb)), "pbf_job_table_info")
            infos.append((nr.value, nb.value, dl.value, kb.value))
            if dl.value + 8 * nb.value + kb.value > 0x7FFFFFFF:
                raise struct.error("'i' format requires -2147483648 <= number <= 2147483647")
        for n, _, _, _ in infos:
            filters.append(BloomFilter(*filter_sizing(n, fp_rate), device=device))
        if any(f.handle is None for f in filters):
            raise ValueError("an output's filter has no bits (fp_rate too large)")
    except BaseException:
        lib.pbf_job_abort(job)
        raise
    nblocks = sum(i[1] for i in infos)
    block_off = np.empty(nblocks + ntables + 1, dtype=np.uint32)
    bounds = np.empty(sum(i[3] for i in infos) + 1, dtype=np.uint8)
    bounds_offs = np.empty(2 * nblocks + 1, dtype=np.uint64)
    handles = (_vp * max(ntables, 1))()
    hs = (_vp * max(ntables, 1))(*[f.handle.value for f in filters])
    _native.check(lib.pbf_job_finish(job, hs, _vp(block_off.ctypes.data), _vp(bounds.ctypes.data),
                                     _vp(bounds_offs.ctypes.data), handles), "pbf_job_finish")
    raw = bounds.tobytes()
    tables, b0, o0 = [], 0, 0
    for t, (n, nb, data_len, _) in enumerate(infos):
        metas = []
        for b in range(nb):
            f0, f1, f2 = (int(x) for x in bounds_offs[2 * (b0 + b):2 * (b0 + b) + 3])
            metas.append((raw[f0:f1].decode("ascii"), raw[f1:f2].decode("ascii"), int(block_off[o0 + b])))
        tables.append(DeviceSSTable._from_handle(_vp(handles[t]), device, metas, filters[t], nb, n, data_len))
        b0 += nb
        o0 += nb + 1
    return tables


def last_stage_ms(device: int) -> dict:
    """Device time of the last finished job on `device` by stage (HIP events), in milliseconds."""
    ms = np.zeros(len(JOB_STAGES), dtype=np.float32)
    _native.check(_native.lib().pbf_job_stage_ms(device, _vp(ms.ctypes.data)), "pbf_job_stage_ms")
    return dict(zip(JOB_STAGES, (float(x) for x in ms)))
