"""Golden compaction outputs at the split rule's edges, from the REAL reference's
``LsmStorage._compact`` (build container only):

    python tools/gen_golden_compaction_edges.py

Writes tests/golden/compaction_split_edges.json, by the recipe of tools/gen_golden_compaction.py
(same fields, same input rules): a split at every finished block, runs that end exactly on a
split / on the single-record closing block / one record after it, one-record blocks, and full
64 KiB blocks.
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
OUT = os.path.join(REPO, "tests", "golden", "compaction_split_edges.json")
sys.path.insert(0, HERE)

from gen_golden_compaction import run  # noqa: E402  (drives the reference's _compact)

CASES = [
    # max_sstable_size 1: every finished block ends its table (40 tables of 4 + 1 records)
    {"name": "split_every_block", "n": 200, "key": "k{i:07d}", "vlen": "48", "block_size": 256, "max_sstable_size": 1},
    # 64-byte records, 256-byte blocks, a split on every 4th block (16 records + the closing one):
    # n = 17 ends with the closing block, 21 leaves four records in an open first block, 22 has
    # one record after a finished block of the second table
    {"name": "ends_on_closing_block", "n": 17, "key": "k{i:07d}", "vlen": "48", "block_size": 256, "max_sstable_size": 1040},
    {"name": "ends_on_split", "n": 21, "key": "k{i:07d}", "vlen": "48", "block_size": 256, "max_sstable_size": 1040},
    {"name": "one_after_split", "n": 22, "key": "k{i:07d}", "vlen": "48", "block_size": 256, "max_sstable_size": 1040},
    # 64..66-byte records into 70-byte blocks: every block holds one record
    {"name": "one_record_blocks", "n": 50, "key": "k{i:07d}", "vlen": "48 + i % 3", "block_size": 70,
     "max_sstable_size": 300},
    # 16-byte records: every block exactly 65536 data bytes, 4096 records
    {"name": "full_64k_blocks", "n": 12289, "key": "{i:04x}", "vlen": "4", "block_size": 65536,
     "max_sstable_size": 100000},
]


def main() -> None:
    cases = []
    for c in CASES:
        outs = run(c)
        covered = outs[-1]["end_record"] if outs else 0
        cases.append(dict(c, outputs=outs, records_written=covered))
        print(c["name"], len(outs), "tables,", covered, "of", c["n"], "records written")
    with open(OUT, "w") as f:
        json.dump({"generator": "tools/gen_golden_compaction_edges.py (reference LsmStorage._compact)",
                   "value_rule": "bytes(((i * 131 + j * 29) & 0xFF) for j in range(vlen))", "cases": cases}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
