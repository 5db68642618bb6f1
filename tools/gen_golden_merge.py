"""Golden compaction runs from the REAL reference's iterators and ``LsmStorage._compact`` (build
container only):

    python tools/gen_golden_merge.py

Writes tests/golden/compaction_merge.json.  For every case of tests/merge_model.py (inputs given
by rule) the input tables are built by the reference's ``SSTableBuilder``, read back by
``SSTableIterator``s, merged by ``MergingIterator`` (force_compaction_l0,
src/lsm_storage.py:253-260) or chained by ``ConcatenatingIterator``
(force_compaction_l1_or_more_level, :272-284), and the run is written by ``_compact``
(:233-251).  Per case: the input rules, the run's record count, the sha256 of its key stream and
of its value stream, the source table of every record (run-length encoded), and per output file
its length and sha256 — hashes and rules only, so the fixture stays small.  The reference's mmh3
dependency is the stand-in of tools/mmh3_shim (see tools/gen_golden.py).
"""
from __future__ import annotations

import hashlib
import itertools
import json
import os
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
OUT = os.path.join(REPO, "tests", "golden", "compaction_merge.json")
sys.path.insert(0, os.path.join(HERE, "mmh3_shim"))
sys.path.insert(1, "/root/reference")
sys.path.insert(2, os.path.join(REPO, "tests"))

from src.iterators import ConcatenatingIterator, MergingIterator, SSTableIterator  # noqa: E402  (the reference)
from src.lsm_storage import LsmStorage  # noqa: E402
from src.sstable import SSTableBuilder  # noqa: E402

import merge_model as MM  # noqa: E402  (the cases' rules)


class Tagged:
    """An iterator that notes which table each record it hands on came from."""

    def __init__(self, inner, table: int, source: dict):
        self.inner, self.table, self.source = inner, table, source

    def __iter__(self):
        return self

    def __next__(self):
        rec = next(self.inner)
        self.source[id(rec)] = self.table
        return rec


def run(case):
    with tempfile.TemporaryDirectory() as d:
        counter = itertools.count()

        def path():
            return os.path.join(d, f"{next(counter):06d}.sst")

        sstables = []
        for rows in MM.case_tables(case):
            b = SSTableBuilder(sstable_size=1 << 22, block_size=case["table_block_size"])
            for k, v in rows:
                b.add(key=k, value=v)
            sstables.append(b.build(path=path()))
        source: dict = {}
        its = [Tagged(SSTableIterator(sstable=t), i, source) for i, t in enumerate(sstables)]
        merged = MergingIterator(iterators=its) if case["mode"] == "merge" else ConcatenatingIterator(iterators=its)
        records = list(merged)  # (kept alive: `source` is keyed by id)
        sources = [source[id(r)] for r in records]
        keys = b"".join(r.key.encode("utf-8") for r in records)
        values = b"".join(r.value for r in records)
        fake = types.SimpleNamespace(
            _configuration=types.SimpleNamespace(max_sstable_size=case["max_sstable_size"],
                                                 block_size=case["block_size"]),
            _compute_path=path)
        outs, written = [], 0
        for t in LsmStorage._compact(fake, iter(records)):
            with open(t.file.path, "rb") as f:
                data = f.read()
            outs.append({"first_key": t.first_key, "last_key": t.last_key, "file_len": len(data),
                         "file_sha256": hashlib.sha256(data).hexdigest()})
            written = [r.key for r in records].index(t.last_key, written) + 1
        return dict(case, input_records=[len(rows) for rows in MM.case_tables(case)], records=len(records),
                    keys_sha256=hashlib.sha256(keys).hexdigest(), values_sha256=hashlib.sha256(values).hexdigest(),
                    source_runs=MM.source_runs(sources), outputs=outs, records_written=written)


def main() -> None:
    cases = []
    for c in MM.CASES:
        g = run(c)
        cases.append(g)
        print(c["name"], g["records"], "records,", len(g["outputs"]), "outputs,", g["records_written"], "written")
    head = {"generator": "tools/gen_golden_merge.py (reference SSTableBuilder, SSTableIterator, "
                         "MergingIterator / ConcatenatingIterator, LsmStorage._compact)",
            "rules": "tests/merge_model.py CASES / case_tables"}
    with open(OUT, "w") as f:  # one case per line (the source runs are long lists)
        f.write(json.dumps(head)[:-1] + ', "cases": [\n')
        f.write(",\n".join(json.dumps(c) for c in cases))
        f.write("\n]}\n")


if __name__ == "__main__":
    main()
