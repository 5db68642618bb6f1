"""Golden memtable reads from the REAL reference's MemTable and LsmStorage (build container only):

    python tools/gen_golden_memtable_read.py

Writes tests/golden/memtable_read.json.

* ``logs``: for every put-log rule of tests/memtable_model.py the reference does ``MemTable.put``
  for every put and ``MemTable.get`` for every probe of ``memtable_read_model.log_probes`` (every
  stored key, absent keys below, between and above, proper prefixes and NUL extensions, the empty
  string).  Kept: hit / miss / stored-empty counts, the sha256 of the hit values and of the hit
  pattern.
* ``store``: a real ``LsmStorage`` (``memtable_read_model.STORE``: a small max_sstable_size, so the
  memtables freeze by themselves; max_l0_sstables large, so nothing compacts by itself; one level)
  is driven to an active memtable, two immutable memtables, three level-0 tables and one level.
  Kept: the put ranges of the memtables, how ``_compact`` split the level, the level tables' first and
  last keys; ``LsmStorage.get`` for every probe of ``store_probes`` with the layer that answered
  (the walk of lsm_storage.py:153-181 redone over the real memtables and tables, asserted equal to
  ``store.get``), run-length encoded; the unbounded ``MemTableIterator`` of each memtable as stream
  hashes; and, for ``scan_model.case_ranges``' rules over the store's scan sources, the store's scan
  AFTER ``close()`` flushed the memtables (real ``SSTable.scan`` + ``MergingIterator`` over the
  resulting level 0), which is what a scan with the memtables as sources must return BEFORE the
  flush.
* For the record only: how many of those (range, memtable) pairs the reference's own
  ``MemTable.scan`` answers incompletely, and the same count for 300 keys inserted ascending,
  descending and shuffled with 300 random ranges each.

The reference's mmh3 dependency is the stand-in of tools/mmh3_shim (see tools/gen_golden.py).
"""
from __future__ import annotations

import hashlib
import json
import os
import random
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
OUT = os.path.join(REPO, "tests", "golden", "memtable_read.json")
sys.path.insert(0, os.path.join(HERE, "mmh3_shim"))
sys.path.insert(1, "/root/reference")
sys.path.insert(2, os.path.join(REPO, "tests"))

from src.iterators import MemTableIterator, SSTableIterator  # noqa: E402  (the reference)
from src.lsm_storage import LsmStorage  # noqa: E402
from src.memtable import MemTable  # noqa: E402

import memtable_model as MT  # noqa: E402  (the put-log rules)
import memtable_read_model as MR  # noqa: E402  (the probe, store and range rules)
import merge_model as MM  # noqa: E402


def sha(parts) -> str:
    return hashlib.sha256(b"".join(parts)).hexdigest()


def run_log(case):
    puts = MT.case_puts(case)
    probes = MR.log_probes(puts)
    with tempfile.TemporaryDirectory() as d:
        memtable = MemTable.create(directory=d)
        for k, v in puts:
            memtable.put(key=k, value=v)
        results = [memtable.get(key=k) for k in probes]
        memtable.wal.file.close()
    model = MR.ModelMemTable(puts)
    assert results == [model.get(k) for k in probes] and memtable.approximate_size == model.approximate_size
    return dict({"name": case["name"], "probes": len(probes), "approximate_size": memtable.approximate_size},
                **MR.probe_digest(results))


def walk(store, key):
    """LsmStorage.get's walk (lsm_storage.py:153-181) with the layer that answered."""
    layer = 0
    for m in [store.state.memtable, *store.state.immutable_memtables]:
        v = m.get(key=key)
        if v is not None:
            return v, layer
        layer += 1
    for t in store.state.sstables_level0:
        if t.bloom_filter.may_contain(key=key):
            v = t.get(key=key)
            if v is not None:
                return v, layer
        layer += 1
    for level in store.state.sstables_levels:
        for t in level:
            if t.first_key <= key <= t.last_key and t.bloom_filter.may_contain(key=key):
                v = t.get(key=key)
                if v is not None:
                    return v, layer
            layer += 1
    return None, -1


def runs(values):
    out = []
    for v in values:
        if out and out[-1][0] == v:
            out[-1][1] += 1
        else:
            out.append([int(v), 1])
    return out


def run_store():
    S = MR.STORE
    with tempfile.TemporaryDirectory() as d:
        os.makedirs(os.path.join(d, "lsm"))  # (create() opens the first WAL before it makes the directory)
        store = LsmStorage.create(max_sstable_size=S["max_sstable_size"], block_size=S["block_size"], max_l0_sstables=100,
                                  nb_levels=1, directory=os.path.join(d, "lsm"))
        p, ranges = 0, []

        def put_until_frozen(count):
            nonlocal p
            first = p
            while count:
                before = len(store.state.immutable_memtables)
                store.put(*MR.store_put(p))
                p += 1
                if len(store.state.immutable_memtables) > before:  # it froze by itself
                    ranges.append([first, p])
                    first = p
                    count -= 1

        put_until_frozen(S["frozen_per_phase"][0])
        for _ in range(S["frozen_per_phase"][0]):
            store.flush_next_immutable_memtable()
        store.force_compaction_l0()
        put_until_frozen(S["frozen_per_phase"][1])
        for _ in range(S["frozen_per_phase"][1]):
            store.flush_next_immutable_memtable()
        put_until_frozen(S["frozen_per_phase"][2])
        for _ in range(S["active_puts"]):
            store.put(*MR.store_put(p))
            p += 1
        ranges.append([p - S["active_puts"], p])
        st = store.state
        assert len(st.immutable_memtables) == 2 and len(st.sstables_level0) == 3 and st.memtable.approximate_size > 0
        assert ranges == MR.store_memtables()

        # how _compact split the level: contiguous slices of the merged run, the tail not written
        level = list(st.sstables_levels[0])
        level_rows = [[(r.key, r.value) for r in SSTableIterator(sstable=t)] for t in level]
        merged = MR.store_layers()[6]
        slices, at = [], 0
        for rows in level_rows:
            assert merged[at:at + len(rows)] == rows
            slices.append([at, len(rows)])
            at += len(rows)
        layers = MR.store_layers(slices)
        mems = [st.memtable, *st.immutable_memtables]
        real = [[(r.key, r.value) for r in MemTableIterator(memtable=m)] for m in mems] + \
               [[(r.key, r.value) for r in SSTableIterator(sstable=t)] for t in st.sstables_level0] + level_rows
        assert real == layers

        probes = MR.store_probes()
        got = [walk(store, k) for k in probes]
        assert [v for v, _ in got] == [store.get(key=k) for k in probes]
        assert got == MR.get_many(layers, probes)
        answered = sorted({u for _, u in got})
        assert answered == [-1] + list(range(len(layers))), answered  # every layer answers somewhere
        shadow = [[sum(1 for k, _ in layers[u] if k in {x for x, _ in layers[w]}) for w in range(u + 1, len(layers))]
                  for u in range(len(layers))]
        # every layer shadows every lower one somewhere (the level's own tables are disjoint)
        assert all(x > 0 for row in shadow[:6] for x in row), shadow

        scan_layers = layers[:6]  # LsmStorage.scan reads the memtables and level 0 only
        rngs = MR.ranges_for(scan_layers)
        short = 0
        for _, lower, upper in rngs:
            for m, rows in zip(mems, layers[:3]):
                if [(r.key, r.value) for r in m.scan(lower=lower, upper=upper)] != MR.in_range(rows, lower, upper):
                    short += 1
        mem_streams = [{"records": len(rows), "keys_sha256": sha(k.encode() for k, _ in rows),
                        "values_sha256": sha(v for _, v in rows)} for rows in layers[:3]]
        store.close()
        assert len(st.sstables_level0) == 6 and not st.immutable_memtables
        flushed = [[(r.key, r.value) for r in SSTableIterator(sstable=t)] for t in st.sstables_level0]
        assert flushed == scan_layers
        scans = []
        for name, lower, upper in rngs:
            recs = [(r.key, r.value) for r in store.scan(lower=lower, upper=upper)]
            want = MR.scan(scan_layers, lower, upper)
            assert [(k.encode(), v) for k, v in recs] == [(k, v) for k, v, _ in want], name
            scans.append({"name": name, "lower": lower, "upper": upper, "records": len(recs),
                          "keys_sha256": sha(k.encode() for k, _ in recs), "values_sha256": sha(v for _, v in recs),
                          "source_runs": MM.source_runs(u for _, _, u in want),
                          "windows": [hi - lo for lo, hi in MR.windows(scan_layers, lower, upper)]})
        for m in [st.memtable]:
            m.wal.file.close()
    return {"rules": S, "memtable_puts": ranges, "level_slices": slices,
            "level_bounds": [[t.first_key, t.last_key] for t in level],
            "layer_records": [len(rows) for rows in layers], "probes": len(probes),
            "answer_runs": runs(u for _, u in got), "get": MR.probe_digest([v for v, _ in got]),
            "memtable_streams": mem_streams, "scans": scans,
            "reference_memtable_scan_short": [short, len(rngs) * 3]}


def tree_scan_bug():
    """For the record: the reference's bounded MemTable.scan over 300 keys inserted ascending,
    descending and shuffled, 300 random ranges each: how many came back short."""
    rnd = random.Random(20240415)
    keys = ["k%04d" % i for i in range(300)]
    orders = [list(keys), list(reversed(keys)), rnd.sample(keys, len(keys))]
    short = total = 0
    for order in orders:
        with tempfile.TemporaryDirectory() as d:
            m = MemTable.create(directory=d)
            for k in order:
                m.put(key=k, value=b"v")
            for _ in range(300):
                a, b = sorted(rnd.sample(range(300), 2))
                got = [r.key for r in m.scan(lower=keys[a], upper=keys[b])]
                short += got != keys[a:b + 1]
                total += 1
            m.wal.file.close()
    return [short, total]


def main() -> None:
    logs = [run_log(c) for c in MT.CASES]
    for g in logs:
        print(g["name"], g["probes"], "probes,", g["hits"], "hits")
    store = run_store()
    print("store:", store["layer_records"], "records per layer,", store["probes"], "probes,", len(store["scans"]),
          "ranges; reference MemTable.scan short on", store["reference_memtable_scan_short"])
    bug = tree_scan_bug()
    print("reference MemTable.scan short on", bug, "random ranges")
    head = {"generator": "tools/gen_golden_memtable_read.py (reference MemTable.put / get, LsmStorage.put / get / "
                         "scan / close, MemTableIterator, SSTableIterator)",
            "rules": "tests/memtable_model.py CASES, tests/memtable_read_model.py log_probes / STORE / store_probes / "
                     "ranges_for",
            "reference_memtable_scan_short_300_keys": bug}
    with open(OUT, "w") as f:
        f.write(json.dumps(head)[:-1] + ', "logs": [\n')
        f.write(",\n".join(json.dumps(c) for c in logs))
        f.write('\n], "store": ')
        f.write(json.dumps(store, ensure_ascii=False))
        f.write("}\n")


if __name__ == "__main__":
    main()
