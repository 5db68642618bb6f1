"""Golden memtable flushes from the REAL reference's MemTable, WAL, MemTableIterator and
SSTableBuilder (build container only):

    python tools/gen_golden_memtable.py

Writes tests/golden/memtable_flush.json.  For every case of tests/memtable_model.py (puts given by
rule) the reference does ``MemTable.put`` for every put (src/memtable.py:64-72), the WAL file's
bytes are read, the memtable is rebuilt from it with ``MemTable.create_from_wal`` (:29-53) and
must equal the first, ``MemTableIterator`` is drained, and the file is built with
``SSTableBuilder`` as ``LsmStorage._do_flush`` does (src/lsm_storage.py:193-205).  Per case: the
rules, the run's record count, the sha256 of its key stream and of its value stream, the sha256 of
the run-length-encoded list of the puts the records came from, and the sha256 and length of the
WAL and of the .sst file — hashes and rules only, so the fixture stays small.  The reference's
mmh3 dependency is the stand-in of tools/mmh3_shim (see tools/gen_golden.py).
"""
from __future__ import annotations

import hashlib
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
OUT = os.path.join(REPO, "tests", "golden", "memtable_flush.json")
sys.path.insert(0, os.path.join(HERE, "mmh3_shim"))
sys.path.insert(1, "/root/reference")
sys.path.insert(2, os.path.join(REPO, "tests"))

from src.iterators import MemTableIterator  # noqa: E402  (the reference)
from src.memtable import MemTable  # noqa: E402
from src.sstable import SSTableBuilder  # noqa: E402

import memtable_model as MT  # noqa: E402  (the cases' rules)


def run(case):
    puts = MT.case_puts(case)
    with tempfile.TemporaryDirectory() as d:
        memtable = MemTable.create(directory=d)
        for k, v in puts:
            memtable.put(key=k, value=v)
        with open(memtable.wal.path, "rb") as f:
            wal = f.read()
        recovered = MemTable.create_from_wal(wal_path=memtable.wal.path)
        assert recovered == memtable and recovered.approximate_size == memtable.approximate_size
        records = list(MemTableIterator(memtable=recovered))
        assert records == list(MemTableIterator(memtable=memtable))
        # the put a record came from: values name their put (memtable_model.value_of), and the
        # model's claim is checked against the record the reference yields
        model = MT.flush_run(puts)
        assert [(r.key.encode("utf-8"), r.value) for r in records] == [(k, v) for k, v, _ in model]
        indices = [i for _, _, i in model]
        assert all(puts[i] == (r.key, r.value) for i, r in zip(indices, records))
        builder = SSTableBuilder(sstable_size=1 << 30, block_size=case["block_size"])
        for r in records:
            builder.add(key=r.key, value=r.value)
        path = os.path.join(d, "flushed.sst")
        builder.build(path=path)
        with open(path, "rb") as f:
            sst = f.read()
        recovered.wal.file.close()
        memtable.wal.file.close()
    return dict(case, records=len(records),
                keys_sha256=hashlib.sha256(b"".join(r.key.encode("utf-8") for r in records)).hexdigest(),
                values_sha256=hashlib.sha256(b"".join(r.value for r in records)).hexdigest(),
                index_sha256=MT.index_hash(indices), wal_len=len(wal), wal_sha256=hashlib.sha256(wal).hexdigest(),
                sst_len=len(sst), sst_sha256=hashlib.sha256(sst).hexdigest())


def main() -> None:
    cases = []
    for c in MT.CASES:
        g = run(c)
        cases.append(g)
        print(c["name"], c["n"], "puts,", g["records"], "records,", g["wal_len"], "WAL bytes,", g["sst_len"], "file bytes")
    head = {"generator": "tools/gen_golden_memtable.py (reference MemTable.put / create_from_wal, WriteAheadLog, "
                         "MemTableIterator, SSTableBuilder as LsmStorage._do_flush)",
            "rules": "tests/memtable_model.py CASES / case_puts"}
    with open(OUT, "w") as f:  # one case per line
        f.write(json.dumps(head)[:-1] + ', "cases": [\n')
        f.write(",\n".join(json.dumps(c) for c in cases))
        f.write("\n]}\n")


if __name__ == "__main__":
    main()
