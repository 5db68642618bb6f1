"""Generate tests/golden/sstable_get.json from the REAL reference's point lookup (build container
only, like the other gen_golden*.py tools):

    python tools/gen_golden_get.py

Single tables: ``SSTableBuilder`` -> file -> ``SSTable.build_from_path(...).get(k)``
(src/sstable.py:175-206) for the record sets and probe lists of tests/sstable_get_model.py.
An LSM: a real ``LsmStorage`` (src/lsm_storage.py:60-85) whose ``state.sstables_level0`` /
``sstables_levels`` hold data-bearing tables built the same way (placed as tools/gen_golden_lsm.py
places its tables), and ``LsmStorage.get(k)`` per probe key; every ``SSTable.get`` is wrapped by a
recorder, so the fixture also holds which tables each get read.

Inputs are given by rule (tests/sstable_get_model.py).  Results: per probe the table (or -1) and
the value's length (one base-36 character each); one sha256 over all returned values in probe order (each prefixed by its
probe index and length); and the sha256 of each value of the probes that make up the four
coverage counts below plus every 64th probe.  The generator asserts, and the fixture records,
that the reference run contains at least 20 keys found in a table that is not their first
candidate, 5 reads of a table that does not hold the key, 20 keys stored in several tables with
different values, and 5 stored empty values.  The reference's mmh3 dependency is the stand-in of
tools/mmh3_shim (see tools/gen_golden.py).
"""
from __future__ import annotations

import hashlib
import json
import os
import struct
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
OUT = os.path.join(REPO, "tests", "golden", "sstable_get.json")
sys.path.insert(0, os.path.join(HERE, "mmh3_shim"))
sys.path.insert(1, "/root/reference")
sys.path.insert(2, os.path.join(REPO, "tests"))

import sstable_get_model as M  # noqa: E402  (the rules; the model itself is not used here)
from src.lsm_storage import LsmStorage  # noqa: E402  (the reference)
from src.sstable import SSTable, SSTableBuilder  # noqa: E402


B36 = "0123456789abcdefghijklmnopqrstuvwxyz"


def build(keys, vals, block_size, path) -> SSTable:
    b = SSTableBuilder(sstable_size=8 << 20, block_size=block_size)
    for k, v in zip(keys, vals):
        b.add(k, v)
    b.build(path)
    return SSTable.build_from_path(path)  # the read path under test (sstable.py:192-206)


def file_facts(path, sst) -> dict:
    with open(path, "rb") as f:
        data = f.read()
    return {"file_len": len(data), "file_sha256": hashlib.sha256(data).hexdigest(),
            "meta_block_offset": sst.meta_block_offset,
            "meta_blocks": [[m.first_key, m.last_key, m.offset] for m in sst.meta_blocks]}


def total_digest(results) -> str:
    h = hashlib.sha256()
    for i, v in enumerate(results):
        if v is not None:
            h.update(struct.pack("<qq", i, len(v)))
            h.update(v)
    return h.hexdigest()


def main():
    doc = {"generated_by": "tools/gen_golden_get.py (reference SSTable.get, src/sstable.py:175-187; "
                           "LsmStorage.get, src/lsm_storage.py:153-181)", "tables": [], "lsm": None}
    with tempfile.TemporaryDirectory() as tmp:
        for name in M.TABLE_CASES:
            keys, vals, bs = M.table_records(name)
            path = os.path.join(tmp, name + ".sst")
            sst = build(keys, vals, bs, path)
            probes = M.table_probes(keys, [(m.first_key, m.last_key, m.offset) for m in sst.meta_blocks])
            got = [sst.get(k) for k in probes]
            stored = dict(zip(keys, vals))
            assert all(g == stored.get(k) for k, g in zip(probes, got)), name
            c = {"name": name, "block_size": bs, "n_records": len(keys), "n_probes": len(probes)}
            c.update(file_facts(path, sst))
            c["found_len"] = [-1 if g is None else len(g) for g in got]
            c["values_sha256"] = total_digest(got)
            c["single_record_blocks"] = sum(m.first_key == m.last_key for m in sst.meta_blocks)
            doc["tables"].append(c)
            print(name, c["file_len"], "bytes,", len(sst.meta_blocks), "blocks,", len(probes), "probes,",
                  sum(g is not None for g in got), "found")

        os.mkdir(os.path.join(tmp, "lsm"))
        store = LsmStorage.create(directory=os.path.join(tmp, "lsm"), nb_levels=2)
        calls: list = []
        tables, holders = [], []
        for t, spec in enumerate(M.LSM_SPECS):
            keys, vals = M.lsm_table_records(spec)
            path = os.path.join(tmp, f"lsm{t}.sst")
            sst = build(keys, vals, M.LSM_BLOCK_SIZE, path)
            real_get = sst.get

            def recorder(key, t=t, real_get=real_get):  # SSTable.get (src/sstable.py:175-187), observed
                v = real_get(key=key)
                calls.append((t, v is not None))
                return v
            sst.get = recorder
            if spec[0] == 0:
                store.state.sstables_level0.append(sst)  # appended in newest-first order
            else:
                store.state.sstables_levels[spec[0] - 1].append(sst)
            facts = file_facts(path, sst)
            facts.update(level=spec[0], first_key=sst.first_key, last_key=sst.last_key, n_records=len(keys))
            del facts["meta_blocks"]  # (checked through the file's sha256)
            tables.append(facts)
            holders.append(dict(zip(keys, vals)))
        probes = M.lsm_probes()
        table, length, results, reads = [], [], [], []
        not_first, misses, multi, empties = [], 0, [], []
        for i, key in enumerate(probes):
            calls.clear()
            v = store.get(key=key)
            results.append(v)
            reads.append([t for t, _ in calls])
            misses += sum(not hit for _, hit in calls)
            if v is None:
                table.append(-1)
                length.append(-1)
                continue
            t = calls[-1][0]
            assert calls[-1][1] and holders[t][key] == v
            table.append(t)
            length.append(len(v))
            if len(calls) > 1:
                not_first.append(i)
            if len({h[key] for h in holders if key in h}) > 1:
                multi.append(i)
            if len(v) == 0:
                empties.append(i)
        counts = {"found_not_in_first_candidate": len(not_first), "reads_of_a_table_without_the_key": misses,
                  "keys_in_several_tables_with_different_values": len(multi), "stored_empty_values_returned": len(empties)}
        assert counts["found_not_in_first_candidate"] >= 20, counts
        assert counts["reads_of_a_table_without_the_key"] >= 5, counts
        assert counts["keys_in_several_tables_with_different_values"] >= 20, counts
        assert counts["stored_empty_values_returned"] >= 5, counts
        detailed = sorted(set(not_first) | set(multi[:40]) | set(empties[:40]) |
                          {i for i in range(0, len(probes), 64) if results[i] is not None})
        doc["lsm"] = {
            "block_size": M.LSM_BLOCK_SIZE, "n_probes": len(probes), "tables": tables, "counts": counts,
            # one character per probe: the table row / the value's length in base 36, "-" = None
            "table_chars": "".join("-" if t < 0 else B36[t] for t in table),
            "len_chars": "".join("-" if n < 0 else B36[n] for n in length),
            "reads": {str(i): r for i, r in enumerate(reads) if len(r) > 1 or (r and table[i] < 0)},
            "not_first": not_first, "multi": multi[:40], "empties": empties[:40],
            "values_sha256": total_digest(results),
            "value_sha256": {str(i): hashlib.sha256(results[i]).hexdigest() for i in detailed},
        }
        print("lsm:", len(tables), "tables,", len(probes), "probes,", counts)
    with open(OUT, "w") as fh:
        json.dump(doc, fh, ensure_ascii=True, separators=(",", ":"))
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
