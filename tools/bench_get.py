"""Batched get, keys in and values out (lsm_get.get_batch's device path), measured per stage.

    python tools/bench_get.py [--tables 8] [--records 1250000] [--probes 10000000] [--steps 5] [--warmup 2]

Shape: 8 SSTables of 1.25M records each (16-byte splitmix hex keys, 40..103-byte values: the
record shape of test_build_sstables_packed_large_run), 4 in L0 (overlapping key ranges) and 4 in
L1 (disjoint ranges); 10M probe keys, half of them stored.  The tables are built by
build_sstable and opened with DeviceSSTable.from_bytes; the probe keys are uploaded once.

Prints one JSON line: HIP-event milliseconds (median of --steps after --warmup) of the filter and
key-range stage, the walk (pbf_sst_get) and the gather (pbf_sst_gather), lookups per second over
the three, the found count, the bytes gathered, and the walk's algorithmic line count: about
log2(blocks) + log2(records per block) 64-byte lines per resolved candidate plus the key and
value bytes, and the bandwidth that count implies at the measured time.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pebbledb_amd import DeviceSSTable, lsm_get  # noqa: E402
from pebbledb_amd.keys import PackedKeys, PackedRecords, splitmix_hex_keys  # noqa: E402
from pebbledb_amd.sstable_data import build_sstable  # noqa: E402


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


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--tables", type=int, default=8)
    ap.add_argument("--records", type=int, default=1_250_000)
    ap.add_argument("--probes", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import torch

    n0 = a.tables // 2
    n1 = a.tables - n0
    t_build = time.time()
    k0 = sorted_keys(1 << 40, n0 * a.records)  # L0: table j holds every n0-th key (overlapping ranges)
    k1 = sorted_keys(2 << 40, n1 * a.records)  # L1: contiguous slices (disjoint ranges)
    parts = [k0[j::n0] for j in range(n0)] + [k1[j * a.records:(j + 1) * a.records] for j in range(n1)]
    tables, nblocks = [], []
    for j, part in enumerate(parts):
        f, metas, _ = build_sstable(records(np.ascontiguousarray(part), j))
        tables.append(DeviceSSTable.from_bytes(f))
        nblocks.append(len(metas))
        del f
    level0, level1 = tables[:n0], tables[n0:]
    rng = np.random.default_rng(7)
    half = a.probes // 2
    stored = np.concatenate([k0, k1])
    present = stored[rng.integers(0, stored.shape[0], half)]
    absent = splitmix_hex_keys(3 << 40, 0, a.probes - half)  # (seeds far apart: key i = splitmix64(seed + i))
    probes = np.concatenate([present, absent])
    probes = np.ascontiguousarray(probes[rng.permutation(a.probes)])
    t_build = time.time() - t_build

    kd = torch.from_numpy(probes.reshape(-1)).cuda()
    torch.cuda.synchronize()
    runs = []
    for step in range(a.warmup + a.steps):
        tm: dict = {}
        table, vals, offs, val_len = lsm_get._walk_device(kd.data_ptr(), 0, 16, a.probes, level0, level1, 0, tm)
        if step >= a.warmup:
            runs.append(tm)
    found = int((table >= 0).sum().item())
    gathered = int(vals.numel())
    med = {k: float(np.median([r[k] for r in runs])) for k in ("filter_ms", "walk_ms", "gather_ms")}
    total_ms = sum(med.values())
    recs_per_block = a.records / (sum(nblocks) / len(nblocks))
    lines = math.log2(sum(nblocks) / len(nblocks)) + math.log2(recs_per_block)
    walk_bytes = found * (lines * 64 + 16) + a.probes * 16
    out = {
        "bench": "get", "tables": a.tables, "records_per_table": a.records, "blocks_per_table": nblocks,
        "probes": a.probes, "steps": a.steps, "warmup": a.warmup,
        "filter_ms": round(med["filter_ms"], 4), "walk_ms": round(med["walk_ms"], 4),
        "gather_ms": round(med["gather_ms"], 4), "total_ms": round(total_ms, 4),
        "lookups_per_s": round(a.probes / (total_ms * 1e-3)), "found": found, "bytes_gathered": gathered,
        "dominant_stage": max(med, key=med.get),
        "walk_lines_per_candidate": round(lines, 2), "walk_algorithmic_bytes": int(walk_bytes),
        "walk_algorithmic_gbps": round(walk_bytes / (med["walk_ms"] * 1e-3) / 1e9, 1),
        "gather_gbps": round(2 * gathered / (med["gather_ms"] * 1e-3) / 1e9, 1),
        "all_runs_ms": runs, "setup_s": round(t_build, 1),
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
