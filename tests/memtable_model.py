"""TEST INFRASTRUCTURE — a plain-Python restatement of a memtable flush's record run, and the
input rules of tests/golden/memtable_flush.json (tools/gen_golden_memtable.py writes that fixture
from the REAL reference with these rules; tests/test_memtable_model_cpu.py pins this model to it).

Restated:
* MemTable.put (src/memtable.py:64-72) appends Record.to_bytes() to the WAL and inserts into a
  red-black tree that replaces the data of a key it already holds (src/red_black_tree.py:118-120);
  MemTableIterator (src/iterators.py:24-55) walks the tree in key order.  So: every distinct key
  once, in key order, with the value of its LAST put.  Here: a dict filled in put order, sorted by
  key bytes (the reference's str order for ASCII keys, the only ones a flush accepts).
* The WAL (src/wal.py:37-38, record.py:66-72): i32 key_size | key | i32 value_size | value of
  every put, back to back, in put order.

A put log is a list of (key, value) pairs in put order; keys are str or bytes.
"""
from __future__ import annotations

import hashlib
import json
import struct

MASK64 = (1 << 64) - 1


def _b(key) -> bytes:
    return key.encode("utf-8") if isinstance(key, str) else bytes(key)


def flush_run(puts):
    """[(key bytes, value, put index)] of MemTableIterator over a memtable that received `puts`."""
    last = {}
    for i, (k, v) in enumerate(puts):
        last[_b(k)] = (v, i)
    return [(k, v, i) for k, (v, i) in sorted(last.items())]


def wal_bytes(puts) -> bytes:
    """The WAL file of a memtable that received `puts`."""
    out = []
    for k, v in puts:
        kb = _b(k)
        out.append(struct.pack("<i", len(kb)) + kb + struct.pack("<i", len(v)) + v)
    return b"".join(out)


def stream_hashes(run) -> tuple[str, str]:
    """sha256 of the run's keys back to back, and of its values."""
    return (hashlib.sha256(b"".join(k for k, _, _ in run)).hexdigest(),
            hashlib.sha256(b"".join(v for _, v, _ in run)).hexdigest())


def index_runs(indices) -> list[list[int]]:
    """Run-length encoding [[first, count], ...] of a put-index list: a run is indices that go up
    by one."""
    out: list[list[int]] = []
    for i in indices:
        i = int(i)
        if out and out[-1][0] + out[-1][1] == i:
            out[-1][1] += 1
        else:
            out.append([i, 1])
    return out


def index_hash(indices) -> str:
    """sha256 of the run-length-encoded put-index list."""
    return hashlib.sha256(json.dumps(index_runs(indices), separators=(",", ":")).encode()).hexdigest()


# ----------------------------------------------------------------------------- fixture rules
def mix(seed: int, i: int) -> int:
    """splitmix64 of (seed << 32) + i."""
    z = (((seed << 32) + i) + 0x9E3779B97F4A7C15) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def value_of(i: int, n: int) -> bytes:
    return bytes(((i * 131 + j * 29) & 0xFF) for j in range(n))


# A case: put i of "n" has key eval(case["key"]) and value value_of(i, eval(case["vlen"])), both
# expressions in i and h = mix(case["seed"], i): a value names its put, so a wrong duplicate shows
# in the value stream.  "block_size" is the flush's SSTableBuilder block size.
CASES = [
    # about 4 puts per key, less than one sort tile
    {"name": "dups_one_tile", "n": 1500, "seed": 1, "key": "'k%05d' % (h % 400)", "vlen": "1 + (i * 7) % 23",
     "block_size": 1024},
    # three sort tiles: one merge pass; values of length 0 among them
    {"name": "dups_three_tiles", "n": 5000, "seed": 2, "key": "'key-%06d' % (h % 3000)", "vlen": "(i * 5) % 41",
     "block_size": 4096},
    # distinct keys put in descending order
    {"name": "distinct_descending", "n": 2500, "seed": 3, "key": "'k%06d' % (99999 - 3 * i)", "vlen": "3 + i % 9",
     "block_size": 2048},
    # every put has the same key: one record, the last put's
    {"name": "same_key", "n": 300, "seed": 4, "key": "'only'", "vlen": "1 + i % 5", "block_size": 1024},
    # keys of 1..27 bytes that share prefixes of every length, many a proper prefix of another
    {"name": "shared_prefixes", "n": 3000, "seed": 5, "key": "'p' * (1 + h % 20) + '%x' % (h // 32 % 90)",
     "vlen": "i % 19", "block_size": 1024},
    # keys that differ only in trailing NUL characters: equal zero-padded prefixes, unequal keys
    {"name": "trailing_nul", "n": 400, "seed": 6, "key": "'ab'[:1 + h % 2] + chr(0) * (h // 2 % 4) + 'c' * (h // 8 % 2)",
     "vlen": "2 + i % 7", "block_size": 512},
]


def case_puts(case):
    """The put log of a case: [(key str, value bytes), ...] in put order."""
    puts = []
    for i in range(case["n"]):
        env = {"i": i, "h": mix(case["seed"], i)}
        puts.append((eval(case["key"], env), value_of(i, eval(case["vlen"], env))))
    return puts
