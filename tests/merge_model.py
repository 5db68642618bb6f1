"""TEST INFRASTRUCTURE — a plain-Python restatement of compaction's record run, and the input
rules of tests/golden/compaction_merge.json (tools/gen_golden_merge.py writes that fixture from
the REAL reference with these rules; tests/test_merge_model_cpu.py pins this model to it).

Restated:
* MergingIterator over SSTableIterators (src/iterators.py:110-190): a heap keyed (key, iterator
  index), then _filter_duplicate_keys, which keeps the first record of a key — so every distinct
  key once, in key order, with the record of the lowest table index that stores it.  Here: fill
  a dict from the oldest table (the last) to the newest (tables[0]), then sort by key bytes.
* ConcatenatingIterator (iterators.py:193-207): every record, table after table.

A table is a list of (key, value) pairs in its own key order; keys are str or bytes (str keys
are compared as their UTF-8 bytes, which is the reference's str order for ASCII keys, the only
ones a resident table holds).
"""
from __future__ import annotations

import hashlib


def _b(key) -> bytes:
    return key.encode("utf-8") if isinstance(key, str) else bytes(key)


def merge(tables):
    """[(key bytes, value, source table)] of MergingIterator(tables)."""
    newest = {}
    for t in range(len(tables) - 1, -1, -1):
        for k, v in tables[t]:
            newest[_b(k)] = (v, t)
    return [(k, v, t) for k, (v, t) in sorted(newest.items())]


def concat(tables):
    """[(key bytes, value, source table)] of ConcatenatingIterator(tables)."""
    return [(_b(k), v, t) for t, table in enumerate(tables) for k, v in table]


def run_of(tables, mode: str):
    return merge(tables) if mode == "merge" else concat(tables)


def stream_hashes(run) -> tuple[str, str]:
    """sha256 of the run's keys back to back, and of its values."""
    return (hashlib.sha256(b"".join(k for k, _, _ in run)).hexdigest(),
            hashlib.sha256(b"".join(v for _, v, _ in run)).hexdigest())


def source_runs(sources) -> list[list[int]]:
    """Run-length encoding [[table, count], ...] of the records' source tables."""
    out: list[list[int]] = []
    for t in sources:
        if out and out[-1][0] == t:
            out[-1][1] += 1
        else:
            out.append([int(t), 1])
    return out


# ----------------------------------------------------------------------------- fixture rules
def value_of(i: int, n: int) -> bytes:
    return bytes(((i * 131 + j * 29) & 0xFF) for j in range(n))


# A case: "tables" = [[first, stop, step, version], ...] (tables[0] the newest); record i of a table
# has key case["key"].format(i=i) and value b"" where case["empty"] holds, else
# value_of(i * 17 + ver, case["vlen"]) — both expressions in i and ver.  "table_block_size" is the
# block size the INPUT tables are built with; "block_size" / "max_sstable_size" are _compact's.
CASES = [
    # 3 tables with overlapping key sets
    {"name": "overlap3", "mode": "merge", "key": "k{i:06d}", "vlen": "1 + (i * 5 + ver * 3) % 29", "empty": "False",
     "tables": [[0, 900, 3, 1], [300, 1500, 2, 2], [100, 1300, 5, 3]],
     "table_block_size": 512, "block_size": 1024, "max_sstable_size": 8192},
    # 5 tables with overlapping key sets, blocks of a few records
    {"name": "overlap5", "mode": "merge", "key": "key-{i:05d}", "vlen": "(i * 7 + ver) % 41", "empty": "False",
     "tables": [[500, 2500, 7, 1], [0, 3000, 4, 2], [1000, 2000, 1, 3], [0, 3000, 6, 4], [2400, 3200, 3, 5]],
     "table_block_size": 256, "block_size": 4096, "max_sstable_size": 20000},
    # every key in every table, a different value (and value length) in each
    {"name": "every_table", "mode": "merge", "key": "k{i:04d}", "vlen": "1 + (i + ver * 11) % 37", "empty": "False",
     "tables": [[0, 300, 1, 4], [0, 300, 1, 3], [0, 300, 1, 2], [0, 300, 1, 1]],
     "table_block_size": 300, "block_size": 1024, "max_sstable_size": 4096},
    # table 1 (older) fully shadowed by table 0; table 2 pokes out on both sides
    {"name": "shadowed", "mode": "merge", "key": "k{i:05d}", "vlen": "2 + (i * 3 + ver * 5) % 23", "empty": "False",
     "tables": [[100, 700, 1, 1], [200, 500, 1, 2], [0, 900, 7, 3]],
     "table_block_size": 400, "block_size": 1024, "max_sstable_size": 6000},
    # empty values in the newest table win over older stored values
    {"name": "empty_newest", "mode": "merge", "key": "k{i:05d}", "vlen": "1 + (i + ver) % 19",
     "empty": "ver == 1 and i % 3 == 0",
     "tables": [[0, 600, 2, 1], [0, 600, 3, 2], [0, 600, 1, 3]],
     "table_block_size": 256, "block_size": 512, "max_sstable_size": 4096},
    # disjoint tables given out of order under concat: list order is kept
    {"name": "concat_out_of_order", "mode": "concat", "key": "k{i:05d}", "vlen": "4 + (i + ver) % 30", "empty": "False",
     "tables": [[1000, 1500, 1, 1], [0, 400, 1, 2], [500, 900, 2, 3]],
     "table_block_size": 512, "block_size": 1024, "max_sstable_size": 8192},
    # a level as force_compaction_l1_or_more_level finds it: disjoint tables in key order
    {"name": "concat_level", "mode": "concat", "key": "k{i:05d}", "vlen": "(i * 3 + ver) % 50", "empty": "False",
     "tables": [[0, 400, 1, 1], [400, 1000, 2, 2], [1000, 1300, 1, 3]],
     "table_block_size": 512, "block_size": 1024, "max_sstable_size": 8192},
    # several outputs; the records after the last split fit one open block and are not written
    # (the merged run is records 0..1083 of compaction_split.json's "tail_dropped")
    {"name": "multi_output_tail_dropped", "mode": "merge", "key": "k{i:08d}", "vlen": "20 + i % 50", "empty": "False",
     "tables": [[0, 1084, 3, 1], [1, 1084, 3, 2], [0, 1084, 2, 3], [2, 1084, 3, 4]],
     "table_block_size": 1024, "block_size": 1024, "max_sstable_size": 16384},
]


def case_tables(case):
    """The input tables of a case: [[(key str, value bytes), ...], ...]."""
    tables = []
    for first, stop, step, ver in case["tables"]:
        rows = []
        for i in range(first, stop, step):
            env = {"i": i, "ver": ver}
            empty = eval(case["empty"], env)
            rows.append((case["key"].format(i=i), b"" if empty else value_of(i * 17 + ver, eval(case["vlen"], env))))
        tables.append(rows)
    return tables
