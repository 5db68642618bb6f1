"""Golden range scans from the REAL reference's bounded iterators (build container only):

    python tools/gen_golden_scan.py

Writes tests/golden/lsm_scan.json.  For every case of tests/scan_model.py (merge_model's table
rules ``overlap3``, ``overlap5``, ``every_table``, ``empty_newest``; ranges by rule,
``scan_model.case_ranges``) the tables are built by the reference's ``SSTableBuilder`` and every
range is read by ``MergingIterator([sstable.scan(lower, upper) for sstable in tables])`` — which
is literally what ``LsmStorage.scan`` constructs (src/lsm_storage.py:187-190) once the memtable
iterators, empty here, are left out.  The case named ``scan_model.LSM_CASE`` is also driven
through a real ``LsmStorage``: its tables are put, frozen and flushed oldest first, so that
``sstables_level0`` holds them in the case's order with empty memtables, and ``storage.scan``
must give the same records as the bare ``MergingIterator`` (asserted here; the fixture notes it).

Per range: the bounds, the record count, the sha256 of the key stream and of the value stream,
the source table of every record (run-length encoded), and per table the number of records its
own ``scan`` yields — hashes and counts only, so the fixture stays small.  The reference's mmh3
dependency is the stand-in of tools/mmh3_shim (see tools/gen_golden.py).

The tables stay far below the ~1000 consecutive out-of-range blocks at which the reference's
``SSTableIterator.__next__`` (one recursion per block that yields nothing) raises RecursionError.
"""
from __future__ import annotations

import hashlib
import itertools
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
OUT = os.path.join(REPO, "tests", "golden", "lsm_scan.json")
sys.path.insert(0, os.path.join(HERE, "mmh3_shim"))
sys.path.insert(1, "/root/reference")
sys.path.insert(2, os.path.join(REPO, "tests"))

from src.iterators import MergingIterator  # noqa: E402  (the reference)
from src.lsm_storage import LsmStorage  # noqa: E402
from src.sstable import SSTableBuilder  # noqa: E402

import merge_model as MM  # noqa: E402  (the cases' table rules)
import scan_model as SM  # noqa: E402  (the cases' range rules)

from gen_golden_merge import Tagged  # noqa: E402


def lsm_storage_scans(case, d, ranges):
    """The case through a real LsmStorage: [(key, value)] per range from storage.scan."""
    os.makedirs(os.path.join(d, "lsm"))  # (create() opens the first WAL before it makes the directory)
    store = LsmStorage.create(max_sstable_size=1 << 22, block_size=case["table_block_size"], max_l0_sstables=100,
                              directory=os.path.join(d, "lsm"))
    for rows in reversed(MM.case_tables(case)):  # oldest first: every flush goes to the front of level 0
        for k, v in rows:
            store.put(key=k, value=v)
        store._freeze_memtable()
        store.flush_next_immutable_memtable()
    assert len(store.state.sstables_level0) == len(case["tables"]) and not store.state.immutable_memtables
    assert store.state.memtable.approximate_size == 0
    return [[(r.key, r.value) for r in store.scan(lower=lo, upper=up)] for _, lo, up in ranges]


def run(case):
    ranges = SM.case_ranges(case)
    with tempfile.TemporaryDirectory() as d:
        counter = itertools.count()
        sstables = []
        for rows in MM.case_tables(case):
            b = SSTableBuilder(sstable_size=1 << 22, block_size=case["table_block_size"])
            for k, v in rows:
                b.add(key=k, value=v)
            sstables.append(b.build(path=os.path.join(d, f"{next(counter):06d}.sst")))
        assert max(len(t.meta_blocks) for t in sstables) < 300
        via_lsm = lsm_storage_scans(case, d, ranges) if case["name"] == SM.LSM_CASE else None
        out = []
        for ri, (name, lower, upper) in enumerate(ranges):
            source: dict = {}
            its = [Tagged(t.scan(lower=lower, upper=upper), i, source) for i, t in enumerate(sstables)]
            records = list(MergingIterator(iterators=its))  # (kept alive: `source` is keyed by id)
            if via_lsm is not None:
                assert via_lsm[ri] == [(r.key, r.value) for r in records], name
            out.append({"name": name, "lower": lower, "upper": upper, "records": len(records),
                        "keys_sha256": hashlib.sha256(b"".join(r.key.encode("utf-8") for r in records)).hexdigest(),
                        "values_sha256": hashlib.sha256(b"".join(r.value for r in records)).hexdigest(),
                        "source_runs": MM.source_runs(source[id(r)] for r in records),
                        "table_records": [sum(1 for _ in t.scan(lower=lower, upper=upper)) for t in sstables]})
        keys = ("name", "key", "vlen", "empty", "tables", "table_block_size")
        return dict({k: case[k] for k in keys}, via_lsm_storage=via_lsm is not None,
                    blocks=[len(t.meta_blocks) for t in sstables], ranges=out)


def main() -> None:
    cases = []
    for c in SM.CASES:
        g = run(c)
        cases.append(g)
        print(c["name"], len(g["ranges"]), "ranges,", sum(r["records"] for r in g["ranges"]), "records",
              "(also through LsmStorage)" if g["via_lsm_storage"] else "")
    head = {"generator": "tools/gen_golden_scan.py (reference SSTableBuilder, SSTable.scan, MergingIterator; "
                         f"{SM.LSM_CASE} also through LsmStorage.scan)",
            "rules": "tests/merge_model.py CASES / case_tables, tests/scan_model.py case_ranges"}
    with open(OUT, "w") as f:  # one case per line
        f.write(json.dumps(head)[:-1] + ', "cases": [\n')
        f.write(",\n".join(json.dumps(c, ensure_ascii=False) for c in cases))
        f.write("\n]}\n")


if __name__ == "__main__":
    main()
