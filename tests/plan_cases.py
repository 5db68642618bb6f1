"""Record-size sequences for the device planner's parity tests (the numpy model on the CPU, the
kernels on the GPU): (name, ko, vo, block_size, max_sstable_size).  Every case is planned in
blocks mode and, with its max_sstable_size, in compaction mode.  A record's encoded size is
key bytes + value bytes + 8."""
from __future__ import annotations

import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CHUNK = 8192  # kPlanChunk


def offsets(sizes, klen=None):
    """(ko, vo) for records of the given encoded sizes: keys of `klen` bytes (default: what is
    left of min(size - 8, 5)), the rest value."""
    sizes = np.asarray(sizes, dtype=np.int64)
    assert sizes.min() >= 8
    kl = np.minimum(sizes - 8, 5 if klen is None else klen)
    vl = sizes - 8 - kl
    ko, vo = np.zeros(len(sizes) + 1, np.uint64), np.zeros(len(sizes) + 1, np.uint64)
    np.cumsum(kl, out=ko[1:])
    np.cumsum(vl, out=vo[1:])
    return ko, vo


def _golden(path):
    out = []
    for c in json.load(open(os.path.join(HERE, "golden", path)))["cases"]:
        kl = [len(c["key"].format(i=i).encode()) for i in range(c["n"])]
        vl = [eval(c["vlen"], {"i": i}) for i in range(c["n"])]
        ko, vo = np.zeros(c["n"] + 1, np.uint64), np.zeros(c["n"] + 1, np.uint64)
        np.cumsum(kl, out=ko[1:])
        np.cumsum(vl, out=vo[1:])
        out.append((path.split(".")[0] + ":" + c["name"], ko, vo, c["block_size"], c["max_sstable_size"]))
    return out


def cases():
    rng = np.random.default_rng(20250)
    u = lambda n, size=64: [size] * n  # noqa: E731
    blk = 4 * 64 + 2 * 4 + 2  # a finished block of four 64-byte records
    out = [
        ("n1", *offsets([20]), 64, 100),
        ("one_record_of_block_size", *offsets([64]), 64, 1),
        ("one_record_of_block_size_then_more", *offsets([64, 64, 9]), 64, 100),
        ("sum_exactly_block_size", *offsets([32, 32] * 10), 64, 200),
        ("sum_one_byte_more", *offsets([32, 33] * 10), 65, 200),
        ("sum_one_byte_more_b", *offsets([32, 33] * 10), 64, 200),
        ("empty_8192_one_block", *offsets([8] * 8192), 65536, 1 << 20),
        ("empty_8193", *offsets([8] * 8193), 65536, 1 << 20),
        ("empty_3x8192_plus5", *offsets([8] * (3 * 8192 + 5)), 65536, 100_000),
        ("block_size_8", *offsets([8] * 300), 8, 50),
        ("block_size_12", *offsets([8 + i % 5 for i in range(300)]), 12, 70),
        ("n_chunk_minus_1", *offsets(rng.integers(8, 90, CHUNK - 1)), 1024, 20_000),
        ("n_chunk", *offsets(rng.integers(8, 90, CHUNK)), 1024, 20_000),
        ("n_chunk_plus_1", *offsets(rng.integers(8, 90, CHUNK + 1)), 1024, 20_000),
        ("block_ends_on_chunk_seam", *offsets(u(3 * CHUNK)), 64 * 128, 100_000),
        ("block_straddles_chunk_seam", *offsets(u(3 * CHUNK)), 64 * 100, 100_000),
        ("open_block_starts_on_chunk_seam", *offsets(u(CHUNK + 17)), 64 * 128, 100_000),
        ("split_every_block", *offsets(u(2 * CHUNK + 3)), 256, 1),
        ("lone_record_is_the_last", *offsets(u(10)), 256, 1),
        ("dropped_tail", *offsets(u(12)), 256, 1),
        ("dropped_tail_long", *offsets(u(5 * 4000 + 3)), 256, 1),
        ("inside_first_open_block", *offsets(u(3)), 256, 1),
        ("position_exactly_max", *offsets(u(40)), 256, 3 * blk),
        ("position_one_under_max", *offsets(u(40)), 256, 3 * blk + 1),
        ("split_crossing_inside_a_late_chunk", *offsets(rng.integers(8, 200, 5 * CHUNK + 77)), 4096, 1_000_003),
        ("large_random", *offsets(rng.integers(8, 120, 300_000)), 4096, 1 << 20),
        ("large_64k_blocks", *offsets(rng.integers(40, 90, 260_000)), 65536, 4 << 20),
        ("large_tiny_tables", *offsets(rng.integers(8, 40, 40_000)), 128, 300),
    ]
    return out + _golden("compaction_split.json") + _golden("compaction_split_edges.json")


OVERSIZE = ("oversize", *offsets([20, 30, 65, 20]), 64, 100)
