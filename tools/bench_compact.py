"""Compaction over resident tables (compaction.merge_tables / compact_l0), measured against the
host path the project offered before it.

    python tools/bench_compact.py [--tables 8] [--records 1000000] [--steps 5] [--warmup 2] [--skip-host]

Shape: 8 SSTables of about 1M records each (16-byte splitmix hex keys, 40..103-byte values, the
record shape of tools/bench_get.py).  The sorted key universe is dealt into tables + 1 classes
and table j holds classes j and j + 1: half of a table's keys are also in the next table, so an
L0 compaction drops (tables - 1) / (2 * tables) of its input.  The tables are built by
build_sstable and opened with DeviceSSTable.from_bytes.

Prints one JSON line:
* merge_ms — ``pbf_sst_merge`` with device outputs, HIP events on the caller's stream around
  the call (median of --steps after --warmup; the call reads three totals back in its middle,
  that wait is inside);
* merge_algorithmic_bytes / merge_gbps / merge_pct_of_hbm_peak — the tables' data sections read
  once plus the packed keys, values and both offsets arrays written once, over merge_ms, against
  8000 GB/s (DESIGN.md §3 "Roofline accounting");
* compact_l0_ms — the whole ``compact_l0`` (merge to host memory, plan, ``pbf_build_sstables``,
  files in host memory), a host clock around the synchronous call (it works on the library's own
  streams, which a caller's events do not bracket);
* compact_l0_resident_ms — ``compact_l0_resident`` on the same tables in the same process, its
  steps alternating with compact_l0's (host clock; the outputs are closed outside the timed part);
  resident_stage_ms — the device time of its last job by stage (HIP events: run, plan, encode,
  filters, validate); resident_to_bytes_ms — ``to_bytes()`` of every output of one step, the file
  download a caller may ask for, timed apart; *_spread_ms — max - min of each path's steps;
* host_path_s — the same run produced on the host from the same file bytes: the records of
  every table decoded in Python, ``heapq.merge`` keyed (key, table), duplicates dropped,
  ``PackedRecords.from_iter`` — once (it takes seconds, not milliseconds), and checked equal to
  the device run.
"""
from __future__ import annotations

import argparse
import ctypes
import heapq
import json
import os
import struct
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pebbledb_amd import DeviceSSTable, _native, compaction  # noqa: E402
from pebbledb_amd.keys import PackedKeys, PackedRecords, splitmix_hex_keys  # noqa: E402
from pebbledb_amd.sstable_data import build_sstable  # noqa: E402

HBM_PEAK_GBPS = 8000.0


def sorted_keys(seed: int, n: int) -> np.ndarray:
    k = splitmix_hex_keys(seed, 0, n)
    return np.sort(np.ascontiguousarray(k).view("S16").reshape(-1)).view(np.uint8).reshape(n, 16)


def records(keys: np.ndarray, salt: int) -> PackedRecords:
    n = keys.shape[0]
    lens = 40 + (np.arange(n, dtype=np.int64) + salt) % 64
    vo = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(lens, out=vo[1:])
    vals = np.resize(((np.arange(251) * 131 + salt) & 0xFF).astype(np.uint8), int(vo[-1]))  # period 251 bytes
    return PackedRecords(PackedKeys.fixed(keys), vals, vo, ascii=True)


def decoded(file_bytes: bytes, metas, data_len: int):
    """SSTableIterator in plain Python: (key, value) of every record, block after block."""
    ends = [m[2] for m in metas[1:]] + [data_len]
    for (_, _, start), end in zip(metas, ends):
        count, = struct.unpack_from("<H", file_bytes, end - 2)
        for o in struct.unpack_from(f"<{count}H", file_bytes, end - 2 - 2 * count):
            ks, = struct.unpack_from("<i", file_bytes, start + o)
            k0 = start + o + 4
            vs, = struct.unpack_from("<i", file_bytes, k0 + ks)
            yield file_bytes[k0:k0 + ks].decode("utf-8"), file_bytes[k0 + ks + 4:k0 + ks + 4 + vs]


def host_merge(files) -> PackedRecords:
    """MergingIterator's run over the files' bytes, on the host."""
    def tagged(j, f, metas, data_len):
        for k, v in decoded(f, metas, data_len):
            yield k, j, v

    def distinct(it):
        last = None
        for k, _, v in it:
            if k != last:
                yield k, v
                last = k

    return PackedRecords.from_iter(distinct(heapq.merge(*[tagged(j, *f) for j, f in enumerate(files)])))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--tables", type=int, default=8)
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-host", action="store_true")
    a = ap.parse_args()
    import torch

    T = a.tables
    t_build = time.time()
    universe = sorted_keys(5 << 40, (T + 1) * a.records // 2)
    cls = np.arange(universe.shape[0]) % (T + 1)
    tables, files = [], []
    for j in range(T):
        part = np.ascontiguousarray(universe[(cls == j) | (cls == j + 1)])
        f, metas, _ = build_sstable(records(part, j))
        t = DeviceSSTable.from_bytes(f)
        tables.append(t)
        files.append((f.tobytes(), metas, t.data_len))
        del f
    t_build = time.time() - t_build
    n_in, nbytes = compaction._bounds(tables)
    data_bytes = sum(t.data_len for t in tables)

    # pbf_sst_merge, device outputs
    vp = ctypes.c_void_p
    keys = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    values = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    ko = torch.empty(n_in + 1, dtype=torch.int64, device="cuda")
    vo = torch.empty(n_in + 1, dtype=torch.int64, device="cuda")
    hs = (vp * T)(*[t.handle.value for t in tables])
    tot = [ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()]
    sp = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    merge_ms = []
    for step in range(a.warmup + a.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = _native.lib().pbf_sst_merge(hs, T, _native.PBF_MERGE_DEDUP, vp(keys.data_ptr()), nbytes, vp(ko.data_ptr()),
                                         vp(values.data_ptr()), nbytes, vp(vo.data_ptr()), n_in + 1,
                                         ctypes.byref(tot[0]), ctypes.byref(tot[1]), ctypes.byref(tot[2]), 1,
                                         vp(sp or None))
        _native.check(rc, "pbf_sst_merge")
        e1.record()
        torch.cuda.synchronize()
        if step >= a.warmup:
            merge_ms.append(e0.elapsed_time(e1))
    n_out, kb, vb = (x.value for x in tot)
    merge_bytes = data_bytes + kb + vb + 2 * 8 * (n_out + 1)

    # the whole compact_l0, and compact_l0_resident on the same tables, step by step in turn
    from pebbledb_amd.resident_write import last_stage_ms

    compact_ms, resident_ms, to_bytes_ms, outs = [], [], [], None
    for step in range(a.warmup + a.steps):
        t0 = time.perf_counter()
        outs, written = compaction.compact_l0(tables)
        dt = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        res, res_written = compaction.compact_l0_resident(tables)
        rdt = (time.perf_counter() - t0) * 1e3
        assert res_written == written and len(res) == len(outs)
        if step >= a.warmup:
            compact_ms.append(dt)
            resident_ms.append(rdt)
        if step == a.warmup + a.steps - 1:
            t0 = time.perf_counter()
            got = [t.to_bytes() for t in res]
            to_bytes_ms.append((time.perf_counter() - t0) * 1e3)
            assert all(np.array_equal(g, f) for g, (f, _, _) in zip(got, outs))
            del got
        for t in res:
            t.close()
    stage_ms = last_stage_ms(tables[0].device)
    out_bytes = sum(len(f) for f, _, _ in outs)

    host_s = None
    if not a.skip_host:
        t0 = time.perf_counter()
        run = host_merge(files)
        host_s = time.perf_counter() - t0
        dev = compaction.merge_tables(tables)
        assert run.n == dev.n == n_out and run.keys.data.tobytes() == dev.keys.data.tobytes()
        assert np.asarray(run.values).tobytes() == np.asarray(dev.values).tobytes()

    med = float(np.median(merge_ms))
    gbps = merge_bytes / (med * 1e-3) / 1e9
    out = {
        "bench": "compact", "tables": T, "records_in": n_in, "records_out": n_out, "key_bytes_out": kb,
        "value_bytes_out": vb, "data_section_bytes_in": data_bytes, "steps": a.steps, "warmup": a.warmup,
        "merge_ms": round(med, 4), "merge_ms_all": [round(x, 4) for x in merge_ms],
        "merge_records_in_per_s": round(n_in / (med * 1e-3)),
        "merge_algorithmic_bytes": int(merge_bytes), "merge_gbps": round(gbps, 1),
        "merge_pct_of_hbm_peak": round(100 * gbps / HBM_PEAK_GBPS, 2),
        "compact_l0_ms": round(float(np.median(compact_ms)), 2), "compact_l0_ms_all": [round(x, 2) for x in compact_ms],
        "compact_l0_outputs": len(outs), "compact_l0_file_bytes": out_bytes, "compact_l0_records_written": written,
        "compact_l0_spread_ms": round(max(compact_ms) - min(compact_ms), 2),
        "compact_l0_resident_ms": round(float(np.median(resident_ms)), 2),
        "compact_l0_resident_ms_all": [round(x, 2) for x in resident_ms],
        "compact_l0_resident_spread_ms": round(max(resident_ms) - min(resident_ms), 2),
        "resident_stage_ms": {k: round(v, 3) for k, v in stage_ms.items()},
        "resident_to_bytes_ms": round(to_bytes_ms[0], 2),
        "host_path_s": None if host_s is None else round(host_s, 2), "setup_s": round(t_build, 1),
    }
    print(json.dumps(out))
    for t in tables:
        t.close()


if __name__ == "__main__":
    main()
