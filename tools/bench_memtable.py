"""The device memtable (pebbledb_amd/device_memtable.py, the ``memtables`` keyword of lsm_get /
lsm_scan), measured per stage and against the two ways the project offered before it.

    python tools/bench_memtable.py [--puts 1000000,4000000] [--probes 10000000] [--tables 8]
                                   [--records 1250000] [--ranges 4096] [--steps 3] [--warmup 1]

Shape: put logs of --puts puts (tools/bench_flush.py's key and value rule: 16-byte splitmix hex
keys, 40..103-byte values, a quarter of the puts repeating a key put before, shuffled); behind the
memtable tools/bench_get.py's 8 tables of 1.25M records; 10M probe keys, half of them stored in
the memtable (memtable-only get) or half of them stored anywhere (the store get); --ranges ranges
of about 1000 keys each over the memtable + the tables.

Prints one JSON line per put-log size.  HIP-event milliseconds are the median of --steps after
--warmup; *_wall_ms are host clocks around the same calls:
* apply_ms — ``put_many`` of the whole log into an empty memtable (upload, sort, prefix; host clock)
  with apply_sort_stage_ms, the device time of its sort chain by stage (HIP events,
  ``pbf_log_sort_stage_ms``: upload, entries, tile sort, merge passes, mark, scans, copy; the run
  stays on the device, so the download stage is empty); apply_second_ms — a second log of a tenth
  of the size into the resident run (sort, merge; host clock) with apply_second_sort_stage_ms, the
  same marks for its batch: the merge with the resident run carries no event marks, it is the
  rest of the host time;
* mt_get — the memtable stage alone (``pbf_mt_get``) and the gather for the 10M probes;
* store_get — ``get_batch`` with the memtable in front of the 8 tables: memtable, filter, walk and
  gather stages;
* baseline_dict — (a) a Python ``dict`` of the puts asked 10M times, then ``get_batch`` over the
  tables for the keys it missed: dict_s is the dict's part alone (host clock, once);
* baseline_flushed — (b) ``flush_log_resident`` of the puts, then ``get_batch`` with that table as
  L0[0]: flush_ms once per store, get stages per batch;
* scan — ``scan_ranges`` of --ranges ranges over the memtable + the tables (host clock: the call
  returns host arrays), against the same ranges with the flushed table in the memtable's place;
* flush_resident_ms — ``DeviceMemTable.flush_resident`` (no upload, no sort) with its job stages.
ratio_vs_dict = baseline_dict total / store_get total, ratio_vs_flushed = baseline_flushed get /
store_get total (above 1: the memtable path is faster).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_flush import STAGES as SORT_STAGES, put_log  # noqa: E402
from bench_get import records, sorted_keys  # noqa: E402
from pebbledb_amd import DeviceMemTable, DeviceSSTable, _native, lsm_get, lsm_scan, memtable  # noqa: E402
from pebbledb_amd.keys import PackedKeys, PackedRecords, splitmix_hex_keys  # noqa: E402
from pebbledb_amd.resident_write import last_stage_ms  # noqa: E402
from pebbledb_amd.sstable_data import build_sstable  # noqa: E402

GET_STAGES = ("memtable_ms", "filter_ms", "walk_ms", "gather_ms")


def med(xs) -> float:
    return round(float(np.median(xs)), 4)


def sort_stages() -> list:
    """Device time of the last pbf_log_sort chain on device 0 by stage (an apply runs one)."""
    import ctypes
    ms = (ctypes.c_float * len(SORT_STAGES))()
    _native.check(_native.lib().pbf_log_sort_stage_ms(0, ms, None), "pbf_log_sort_stage_ms")
    return list(ms)


def get_stages(kd, n, level0, level1, mts, steps, warmup):
    """Median HIP-event stage times and wall time of the device get over the uploaded probes."""
    import torch
    runs, wall, table = [], [], None
    for step in range(warmup + steps):
        tm: dict = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        table, _, _, _ = lsm_get._walk_device(kd.data_ptr(), 0, 16, n, level0, level1, 0, tm, memtables=mts)
        dt = (time.perf_counter() - t0) * 1e3
        if step >= warmup:
            runs.append(tm)
            wall.append(dt)
    out = {k: med([r[k] for r in runs]) for k in GET_STAGES if k in runs[0]}
    out["total_ms"] = round(sum(out.values()), 4)
    out["wall_ms"] = med(wall)
    return out, table


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--puts", default="1000000,4000000")
    ap.add_argument("--probes", type=int, default=10_000_000)
    ap.add_argument("--tables", type=int, default=8)
    ap.add_argument("--records", type=int, default=1_250_000)
    ap.add_argument("--ranges", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--skip-dict", action="store_true")
    a = ap.parse_args()
    import torch

    # bench_get.py's tables
    t0 = time.time()
    n0 = a.tables // 2
    n1 = a.tables - n0
    k0 = sorted_keys(1 << 40, n0 * a.records)
    k1 = sorted_keys(2 << 40, n1 * a.records)
    parts = [k0[j::n0] for j in range(n0)] + [k1[j * a.records:(j + 1) * a.records] for j in range(n1)]
    tables = []
    for j, part in enumerate(parts):
        f, _, _ = build_sstable(records(np.ascontiguousarray(part), j))
        tables.append(DeviceSSTable.from_bytes(f))
        del f
    level0, level1 = tables[:n0], tables[n0:]
    table_keys = np.concatenate([k0, k1])
    setup_s = time.time() - t0
    rng = np.random.default_rng(7)

    for nputs in [int(x) for x in a.puts.split(",")]:
        log, distinct = put_log(nputs, 0.25)
        second, _ = put_log(max(1, nputs // 10), 0.25, seed=12)
        mt_keys = log.keys.data.reshape(-1, 16)

        apply_ms, second_ms, apply_st, second_st = [], [], [], []
        mt = None
        for step in range(a.warmup + a.steps):
            if mt is not None:
                mt.close()
            mt = DeviceMemTable()
            t0 = time.perf_counter()
            mt.put_many(log)
            apply_ms.append((time.perf_counter() - t0) * 1e3)
            apply_st.append(sort_stages())
            if step < a.warmup + a.steps - 1:  # the last memtable keeps the first log alone
                t0 = time.perf_counter()
                mt.put_many(second)
                second_ms.append((time.perf_counter() - t0) * 1e3)
                second_st.append(sort_stages())
        assert len(mt) == distinct

        # the memtable alone: 10M probes, half of them stored in it
        half = a.probes // 2
        absent = splitmix_hex_keys(3 << 40, 0, a.probes - half)
        p_mt = np.concatenate([mt_keys[rng.integers(0, nputs, half)], absent])
        p_mt = np.ascontiguousarray(p_mt[rng.permutation(a.probes)])
        kd = torch.from_numpy(p_mt.reshape(-1)).cuda()
        mt_get, table = get_stages(kd, a.probes, [], [], [mt], a.steps, a.warmup)
        mt_get["found"] = int((table != -1).sum().item())
        del kd

        # the store: a quarter in the memtable, a quarter in the tables, half nowhere
        q = a.probes // 4
        p_st = np.concatenate([mt_keys[rng.integers(0, nputs, q)], table_keys[rng.integers(0, table_keys.shape[0], q)],
                               splitmix_hex_keys(4 << 40, 0, a.probes - 2 * q)])
        p_st = np.ascontiguousarray(p_st[rng.permutation(a.probes)])
        kd = torch.from_numpy(p_st.reshape(-1)).cuda()
        store_get, table = get_stages(kd, a.probes, level0, level1, [mt], a.steps, a.warmup)
        store_get["found_memtable"] = int((table <= -2).sum().item())
        store_get["found_tables"] = int((table >= 0).sum().item())

        # (b) the puts flushed to a table that stands as L0[0]
        t0 = time.perf_counter()
        flushed = memtable.flush_log_resident(log)
        flush_b_ms = (time.perf_counter() - t0) * 1e3
        base_b, tb = get_stages(kd, a.probes, [flushed] + level0, level1, [], a.steps, a.warmup)
        assert int((tb == 0).sum().item()) == store_get["found_memtable"]
        assert int((tb > 0).sum().item()) == store_get["found_tables"]
        base_b["flush_ms"] = round(flush_b_ms, 3)

        # (a) a Python dict in front of get_batch
        base_a = None
        if not a.skip_dict:
            kb, vb, vo = log.keys.data.tobytes(), np.asarray(log.values).tobytes(), log.value_offsets
            d = {}
            for i in range(nputs):
                d[kb[16 * i:16 * i + 16]] = vb[int(vo[i]):int(vo[i + 1])]
            pb = p_st.tobytes()
            keys = [pb[16 * i:16 * i + 16] for i in range(a.probes)]
            t0 = time.perf_counter()
            got = [d.get(k) for k in keys]
            dict_s = time.perf_counter() - t0
            miss = np.fromiter((g is None for g in got), dtype=bool, count=a.probes)
            assert int((~miss).sum()) == store_get["found_memtable"]
            km = torch.from_numpy(np.ascontiguousarray(p_st[miss]).reshape(-1)).cuda()
            rest, _ = get_stages(km, int(miss.sum()), level0, level1, [], a.steps, a.warmup)
            base_a = {"dict_s": round(dict_s, 3), "dict_build_excluded": True, "tables_get": rest,
                      "total_ms": round(dict_s * 1e3 + rest["total_ms"], 3)}
            del d, keys, got, km

        # 4096 ranges of about 1000 keys over the memtable + the tables
        # (put_log draws its keys from splitmix_hex_keys(7 << 40, 0, distinct): the memtable's key set)
        allk = np.sort(np.concatenate([table_keys, splitmix_hex_keys(7 << 40, 0, distinct)]).view("S16").reshape(-1))
        starts = rng.integers(0, allk.shape[0] - 1001, a.ranges)
        ranges = [(allk[s].decode(), allk[s + 1000].decode()) for s in starts]
        scan_ms, scan_b_ms, nrec = [], [], 0
        for step in range(a.warmup + a.steps):
            t0 = time.perf_counter()
            pr, _ = lsm_scan.scan_ranges(level0, ranges, memtables=[mt])
            dt = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            pb_, _ = lsm_scan.scan_ranges([flushed] + level0, ranges)
            dtb = (time.perf_counter() - t0) * 1e3
            assert pr.n == pb_.n
            nrec = pr.n
            if step >= a.warmup:
                scan_ms.append(dt)
                scan_b_ms.append(dtb)
        flushed.close()

        fr_ms, t = [], None
        for step in range(a.warmup + a.steps):
            t0 = time.perf_counter()
            t = mt.flush_resident()
            dt = (time.perf_counter() - t0) * 1e3
            if step >= a.warmup:
                fr_ms.append(dt)
            t.close()
        out = {
            "bench": "memtable", "puts": nputs, "records": distinct, "probes": a.probes, "tables": a.tables,
            "records_per_table": a.records, "steps": a.steps, "warmup": a.warmup,
            "apply_ms": med(apply_ms[a.warmup:]), "apply_ms_all": [round(x, 3) for x in apply_ms],
            "apply_sort_stage_ms": dict(zip(SORT_STAGES, (med(x) for x in zip(*apply_st[a.warmup:])))),
            "apply_second_puts": second.n, "apply_second_ms": med(second_ms[a.warmup:] or second_ms),
            "apply_second_sort_stage_ms": dict(zip(SORT_STAGES, (med(x) for x in zip(*(second_st[a.warmup:] or second_st))))),
            "mt_get": mt_get, "store_get": store_get, "baseline_flushed": base_b, "baseline_dict": base_a,
            "ratio_vs_flushed": round(base_b["total_ms"] / store_get["total_ms"], 3),
            "ratio_vs_dict": None if base_a is None else round(base_a["total_ms"] / store_get["total_ms"], 2),
            "scan": {"ranges": a.ranges, "records": nrec, "memtable_ms": med(scan_ms), "flushed_table_ms": med(scan_b_ms)},
            "flush_resident_ms": med(fr_ms), "flush_resident_stage_ms": {k: round(v, 4) for k, v in last_stage_ms(0).items()},
            "setup_s": round(setup_s, 1),
        }
        print(json.dumps(out), flush=True)
        mt.close()
        del kd


if __name__ == "__main__":
    main()
