"""Range scans over resident tables (lsm_scan.scan_ranges / pbf_sst_scan), measured against the
compaction merge in the same process and against the host path the project offered before.

    python tools/bench_scan.py [--tables 8] [--records 1000000] [--ranges 4096] [--range-keys 1000]
                               [--steps 5] [--warmup 2] [--host-ranges 4096] [--skip-host] [--out FILE]

Shape: the 8 resident tables of tools/bench_compact.py (about 1M records each, 16-byte splitmix
hex keys, 40..103-byte values, half of each table's keys also in the next table).

Prints (and with --out writes) one JSON line:
* (a) open_scan_ms / merge_ms — one open range ("", "") through ``pbf_sst_scan`` and
  ``pbf_sst_merge`` over the same tables, alternating, device outputs, HIP events on the
  caller's stream around each call (median of --steps after --warmup; each call reads its totals
  back in its middle, that wait is inside).  The merge's kernels are the baseline; the scan adds
  the bounds stage, the segment scan and one segment search per record.  ``merge_spread_ms`` is
  the merge's max - min over its timed runs.
* (b) ranges_ms — --ranges ranges of --range-keys consecutive keys of the sorted universe, every
  second one shifted to overlap the one before it by half, in one ``pbf_sst_scan`` call (device
  outputs, HIP events); ``size_ms`` is the ``pbf_sst_scan_size`` call that gives its capacities
  (synchronous, a host clock).  ranges_per_s / records_out_per_s are over ranges_ms.
* (c) host_ranges_s — the host path for the first --host-ranges ranges of (b): the records of
  every table decoded in Python from the file bytes (host_decode_s, once), then per range
  ``bisect`` over every table's keys and ``heapq.merge`` keyed (key, table), duplicates dropped.
  Its key and value streams are checked equal to the device run's by sha256.
"""
from __future__ import annotations

import argparse
import ctypes
import hashlib
import heapq
import json
import os
import sys
import time
from bisect import bisect_left, bisect_right

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_compact import decoded, records, sorted_keys  # noqa: E402  (the tables' shape)

from pebbledb_amd import DeviceSSTable, _native, compaction  # noqa: E402
from pebbledb_amd.lsm_scan import _Bounds  # noqa: E402
from pebbledb_amd.sstable_data import build_sstable  # noqa: E402

vp = ctypes.c_void_p


def host_ranges(tables_kv, ranges):
    """The runs of `ranges` on the host: (records, sha256 of the key stream, of the value stream)."""
    hk, hv, n = hashlib.sha256(), hashlib.sha256(), 0

    def window(j, keys, vals, lo, hi):
        for i in range(lo, hi):
            yield keys[i], j, vals[i]

    for lower, upper in ranges:
        its = []
        for j, (keys, vals) in enumerate(tables_kv):
            lo = bisect_left(keys, lower)
            hi = bisect_right(keys, upper) if upper else len(keys)
            its.append(window(j, keys, vals, lo, max(lo, hi)))
        last = None
        for k, _, v in heapq.merge(*its):
            if k != last:
                hk.update(k.encode("utf-8"))
                hv.update(v)
                n += 1
                last = k
    return n, hk.hexdigest(), hv.hexdigest()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--tables", type=int, default=8)
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--ranges", type=int, default=4096)
    ap.add_argument("--range-keys", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-ranges", type=int, default=4096)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--out")
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
    hs = (vp * T)(*[t.handle.value for t in tables])
    L = _native.lib()
    sp = torch.cuda.current_stream().cuda_stream

    # the ranges of (b): pairs of ranges that share half their keys, the pairs apart from each other
    U, W, Q = universe.shape[0], a.range_keys, a.ranges
    stride = max(U // max((Q + 1) // 2, 1), 1)
    assert stride >= W + W // 2 and ((Q - 1) // 2) * stride + W + W // 2 <= U, "the ranges do not fit the universe"
    ukey = lambda i: universe[i].tobytes().decode()  # noqa: E731
    ranges = []
    for q in range(Q):
        first = (q // 2) * stride + (W // 2 if q % 2 else 0)
        ranges.append((ukey(first), ukey(first + W - 1)))

    def buffers(n, kbytes, vbytes, nranges):
        return (torch.empty(max(kbytes, 1), dtype=torch.uint8, device="cuda"),
                torch.empty(max(vbytes, 1), dtype=torch.uint8, device="cuda"),
                torch.empty(n + 1, dtype=torch.int64, device="cuda"), torch.empty(n + 1, dtype=torch.int64, device="cuda"),
                torch.empty(nranges + 1, dtype=torch.int64, device="cuda"))

    def sizes(b):
        tot = [ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()]
        t0 = time.perf_counter()
        _native.check(L.pbf_sst_scan_size(hs, T, *b.args(), None, None, *[ctypes.byref(x) for x in tot]), "pbf_sst_scan_size")
        return [x.value for x in tot], (time.perf_counter() - t0) * 1e3

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    # (a) one open range against the merge, alternating
    keys, values, ko, vo, ro = buffers(n_in, nbytes, nbytes, 1)
    tot = [ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()]
    byref = [ctypes.byref(x) for x in tot]
    one = _Bounds([("", "")])

    def merge():
        _native.check(L.pbf_sst_merge(hs, T, _native.PBF_MERGE_DEDUP, vp(keys.data_ptr()), nbytes, vp(ko.data_ptr()),
                                      vp(values.data_ptr()), nbytes, vp(vo.data_ptr()), n_in + 1, *byref, 1,
                                      vp(sp or None)), "pbf_sst_merge")

    def open_scan():
        _native.check(L.pbf_sst_scan(hs, T, *one.args(), vp(keys.data_ptr()), nbytes, vp(ko.data_ptr()),
                                     vp(values.data_ptr()), nbytes, vp(vo.data_ptr()), n_in + 1, *byref,
                                     vp(ro.data_ptr()), 1, vp(sp or None)), "pbf_sst_scan")

    torch.cuda.synchronize()
    merge_ms, scan_ms, digests = [], [], {}
    for step in range(a.warmup + a.steps):
        for name, call, out in (("merge", merge, merge_ms), ("scan", open_scan, scan_ms)):
            ms = timed(call)
            if step >= a.warmup:
                out.append(ms)
            if step == 0:
                n_out, kb, vb = (x.value for x in tot)
                digests[name] = (n_out, hashlib.sha256(keys[:kb].cpu().numpy().tobytes()).hexdigest(),
                                 hashlib.sha256(values[:vb].cpu().numpy().tobytes()).hexdigest(),
                                 hashlib.sha256(ko[:n_out + 1].cpu().numpy().tobytes()).hexdigest())
    assert digests["merge"] == digests["scan"], "the open scan is not the merge"
    n_merged = digests["merge"][0]
    del keys, values, ko, vo, ro

    # (b) the batch of ranges
    b = _Bounds(ranges)
    (rn, rkb, rvb), _ = sizes(b)
    size_ms = [sizes(b)[1] for _ in range(a.steps)]
    keys, values, ko, vo, ro = buffers(rn, rkb, rvb, Q)

    def batch():
        _native.check(L.pbf_sst_scan(hs, T, *b.args(), vp(keys.data_ptr()), rkb, vp(ko.data_ptr()), vp(values.data_ptr()),
                                     rvb, vp(vo.data_ptr()), rn + 1, *byref, vp(ro.data_ptr()), 1, vp(sp or None)),
                      "pbf_sst_scan")

    ranges_ms = [timed(batch) for _ in range(a.warmup + a.steps)][a.warmup:]
    out_n, out_kb, out_vb = (x.value for x in tot)
    offs = ro.cpu().numpy()
    assert offs[0] == 0 and offs[-1] == out_n and (np.diff(offs) >= 0).all()
    nh = min(a.host_ranges, Q)
    end_rec = int(offs[nh])
    dev_hash = (end_rec, hashlib.sha256(keys[:int(ko[end_rec])].cpu().numpy().tobytes()).hexdigest(),
                hashlib.sha256(values[:int(vo[end_rec])].cpu().numpy().tobytes()).hexdigest())

    # (c) the host path
    host_decode_s = host_s = None
    if not a.skip_host:
        t0 = time.perf_counter()
        tables_kv = []
        for f, metas, data_len in files:
            ks, vs = [], []
            for k, v in decoded(f, metas, data_len):
                ks.append(k)
                vs.append(v)
            tables_kv.append((ks, vs))
        host_decode_s = time.perf_counter() - t0
        t0 = time.perf_counter()
        host_hash = host_ranges(tables_kv, ranges[:nh])
        host_s = time.perf_counter() - t0
        assert host_hash == dev_hash, "the device run is not the host path's"

    med, mmed, rmed = float(np.median(scan_ms)), float(np.median(merge_ms)), float(np.median(ranges_ms))
    out = {
        "bench": "scan", "tables": T, "records_in": n_in, "steps": a.steps, "warmup": a.warmup,
        "open_scan_ms": round(med, 4), "open_scan_ms_all": [round(x, 4) for x in scan_ms],
        "merge_ms": round(mmed, 4), "merge_ms_all": [round(x, 4) for x in merge_ms],
        "merge_spread_ms": round(max(merge_ms) - min(merge_ms), 4), "open_scan_over_merge": round(med / mmed, 4),
        "open_records_out": n_merged, "open_scan_equals_merge_sha256": True,
        "ranges": Q, "range_keys": W, "ranges_records_in": rn, "ranges_records_out": out_n,
        "ranges_key_bytes_out": out_kb, "ranges_value_bytes_out": out_vb,
        "ranges_ms": round(rmed, 4), "ranges_ms_all": [round(x, 4) for x in ranges_ms],
        "size_ms": round(float(np.median(size_ms)), 4),
        "ranges_per_s": round(Q / (rmed * 1e-3)), "records_out_per_s": round(out_n / (rmed * 1e-3)),
        "host_ranges": None if host_s is None else nh, "host_records_out": None if host_s is None else end_rec,
        "host_decode_s": None if host_s is None else round(host_decode_s, 2),
        "host_ranges_s": None if host_s is None else round(host_s, 2),
        "host_equals_device_sha256": None if host_s is None else True,
        "setup_s": round(t_build, 1),
    }
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    for t in tables:
        t.close()


if __name__ == "__main__":
    main()
