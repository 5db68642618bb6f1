"""The device memtable flush (memtable.sort_log / flush_log), measured against the host path the
project offered before it.

    python tools/bench_flush.py [--records 1000000] [--dup 0.25] [--steps 5] [--warmup 2] [--skip-host]

Shape: one put log of --records puts: 16-byte splitmix hex keys, 40..103-byte values (the record
shape of tools/bench_get.py), a --dup share of the puts repeating a key put before, in shuffled
order.

Prints one JSON line:
* stage_ms — device time of ``pbf_log_sort`` by stage, HIP events on the call's stream
  (``pbf_log_sort_stage_ms``; median of --steps after --warmup): upload of the log, k_mt_entries,
  k_mt_tile_sort, the merge passes together, k_mt_mark, the scans and offsets (the read-back of
  the totals between them is inside), k_mt_copy, download of the run;
* sort_log_ms — the whole synchronous ``sort_log`` call (host memory in, host memory out), a host
  clock; flush_log_ms — ``sort_log`` plus ``build_sstable``: the file in host memory;
* flush_log_resident_ms — ``flush_log_resident`` on the same log in the same process, its steps
  alternating with flush_log's (host clock; the table is closed outside the timed part);
  resident_stage_ms — the device time of its last job by stage (HIP events: run, with the log's
  upload; plan; encode; filters; validate); resident_to_bytes_ms — ``to_bytes()`` of the table,
  the file download a caller may ask for, timed apart; *_spread_ms — max - min of a path's steps;
* host_path_s — the same run produced on the host from the same puts as (str, bytes) pairs:
  Python ``dict`` (last put wins), ``sorted``, ``PackedRecords.from_iter`` — once, and checked
  equal to the device run; sort_log_speedup = host_path_s / sort_log_ms.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pebbledb_amd import _native, memtable  # noqa: E402
from pebbledb_amd.keys import PackedKeys, PackedRecords, splitmix_hex_keys  # noqa: E402

STAGES = ("upload", "k_mt_entries", "k_mt_tile_sort", "k_mt_merge_rank", "k_mt_mark", "scans_offsets", "k_mt_copy",
          "download")


def put_log(n: int, dup: float, seed: int = 11):
    """(PackedRecords in put order, the same puts as [(str, bytes)])."""
    rng = np.random.default_rng(seed)
    distinct = max(1, n - int(n * dup))
    ids = np.concatenate([np.arange(distinct), rng.integers(0, distinct, n - distinct)])
    rng.shuffle(ids)
    keys = np.ascontiguousarray(splitmix_hex_keys(7 << 40, 0, distinct)[ids])
    lens = 40 + np.arange(n, dtype=np.int64) % 64
    vo = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(lens, out=vo[1:])
    vals = np.resize(((np.arange(251) * 131 + 7) & 0xFF).astype(np.uint8), int(vo[-1]))  # period 251 bytes
    return PackedRecords(PackedKeys.fixed(keys), vals, vo, ascii=True), distinct


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--dup", type=float, default=0.25)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-host", action="store_true")
    a = ap.parse_args()
    n = a.records
    t0 = time.time()
    log, distinct = put_log(n, a.dup)
    setup_s = time.time() - t0

    sort_ms, stage_ms, passes = [], [], ctypes.c_uint32()
    run = None
    for step in range(a.warmup + a.steps):
        t0 = time.perf_counter()
        run = memtable.sort_log(log)
        dt = (time.perf_counter() - t0) * 1e3
        ms = (ctypes.c_float * len(STAGES))()
        _native.check(_native.lib().pbf_log_sort_stage_ms(0, ms, ctypes.byref(passes)), "pbf_log_sort_stage_ms")
        if step >= a.warmup:
            sort_ms.append(dt)
            stage_ms.append(list(ms))
    assert run.n == distinct

    from pebbledb_amd.resident_write import last_stage_ms

    flush_ms, resident_ms, to_bytes_ms, file_len = [], [], 0.0, 0
    for step in range(a.warmup + a.steps):
        t0 = time.perf_counter()
        f, _, _ = memtable.flush_log(log)
        dt = (time.perf_counter() - t0) * 1e3
        file_len = len(f)
        t0 = time.perf_counter()
        table = memtable.flush_log_resident(log)
        rdt = (time.perf_counter() - t0) * 1e3
        if step >= a.warmup:
            flush_ms.append(dt)
            resident_ms.append(rdt)
        if step == a.warmup + a.steps - 1:
            t0 = time.perf_counter()
            got = table.to_bytes()
            to_bytes_ms = (time.perf_counter() - t0) * 1e3
            assert np.array_equal(got, f)
        table.close()
    res_stage_ms = last_stage_ms(0)

    host_s = None
    if not a.skip_host:
        kb, vb, vo = log.keys.data.tobytes(), np.asarray(log.values).tobytes(), log.value_offsets
        puts = [(kb[16 * i:16 * i + 16].decode(), vb[int(vo[i]):int(vo[i + 1])]) for i in range(n)]
        t0 = time.perf_counter()
        last = {}
        for k, v in puts:
            last[k] = v
        host = PackedRecords.from_iter(sorted(last.items()))
        host_s = time.perf_counter() - t0
        assert host.n == run.n and host.keys.data.tobytes() == run.keys.data.tobytes()
        assert np.asarray(host.values).tobytes() == np.asarray(run.values).tobytes()

    med = float(np.median(sort_ms))
    stages = np.median(np.asarray(stage_ms), axis=0)
    out = {
        "bench": "flush", "puts": n, "dup_share": a.dup, "records_out": run.n, "key_bytes_in": int(log.keys.data.size),
        "value_bytes_in": int(log.value_offsets[-1]), "steps": a.steps, "warmup": a.warmup,
        "fan_in": memtable.FAN_IN, "merge_passes": passes.value,
        "stage_ms": {s: round(float(x), 4) for s, x in zip(STAGES, stages)},
        "device_ms": round(float(stages.sum()), 4), "kernels_ms": round(float(stages[1:7].sum()), 4),
        "sort_log_ms": round(med, 3), "sort_log_ms_all": [round(x, 3) for x in sort_ms],
        "sort_log_puts_per_s": round(n / (med * 1e-3)),
        "flush_log_ms": round(float(np.median(flush_ms)), 3), "flush_log_file_bytes": file_len,
        "flush_log_ms_all": [round(x, 3) for x in flush_ms],
        "flush_log_spread_ms": round(max(flush_ms) - min(flush_ms), 3),
        "flush_log_resident_ms": round(float(np.median(resident_ms)), 3),
        "flush_log_resident_ms_all": [round(x, 3) for x in resident_ms],
        "flush_log_resident_spread_ms": round(max(resident_ms) - min(resident_ms), 3),
        "resident_stage_ms": {k: round(v, 4) for k, v in res_stage_ms.items()},
        "resident_to_bytes_ms": round(to_bytes_ms, 3),
        "host_path_s": None if host_s is None else round(host_s, 3),
        "sort_log_speedup": None if host_s is None else round(host_s / (med * 1e-3), 1),
        "setup_s": round(setup_s, 1),
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
