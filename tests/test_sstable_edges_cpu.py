"""The write side at its limits, host half: the oracle restatement and both block / compaction
planners (numpy and C) pinned to files the REAL reference wrote for record sets at the encoder's
edges (tests/golden/sstable_build_edges.json, tools/gen_golden_sstable_edges.py;
tests/golden/compaction_split_edges.json, tools/gen_golden_compaction_edges.py): a block of
exactly 65536 data bytes, one a byte under, 8192 records in a block (81922 encoded bytes), one
record per block, 12-byte blocks, keys of 1..4-byte code points at every 16-byte residue; a
compaction split at every block, runs ending on / just after a split, full 64 KiB blocks."""
import hashlib
import json
import os

import numpy as np
import pytest

from oracle import sstable_oracle as so
from oracle.oracle import sizing
from pebbledb_amd.keys import PackedKeys
from pebbledb_amd.sstable_data import (key_offsets, meta_blocks, pack_values, plan_blocks, plan_blocks_native,
                                       plan_compaction, plan_compaction_native)

from test_compaction_cpu import case_records

HERE = os.path.dirname(__file__)


def sstable_edge_cases():
    cases = json.load(open(os.path.join(HERE, "golden", "sstable_build_edges.json")))["cases"]
    for c in cases:
        recs = eval(c["records"])  # the generator's rule
        c["_keys"] = [k for k, _ in recs]
        c["_vals"] = [v for _, v in recs]
    return cases


def key_entry(k: str):
    """A meta block's key as the golden file stores it (long keys as sizes + sha256)."""
    if len(k) <= 64:
        return k
    b = k.encode("utf-8")
    return {"chars": len(k), "bytes": len(b), "sha256": hashlib.sha256(b).hexdigest()}


def golden_metas(case):
    return [(m["first_key"], m["last_key"], m["offset"]) for m in case["meta_blocks"]]


SST_CASES = sstable_edge_cases()
SST_IDS = [c["name"] for c in SST_CASES]
COMPACTION_CASES = json.load(open(os.path.join(HERE, "golden", "compaction_split_edges.json")))["cases"]
COMPACTION_IDS = [c["name"] for c in COMPACTION_CASES]


def test_golden_cases_reach_the_limits():
    """The record sets are what the issue lists: the shapes, not only the names."""
    by = {c["name"]: c for c in SST_CASES}
    want = {"full_4096x16": (73822, 2), "off_by_one": (73753, 2), "one_big_value": (65568, 3),
            "big_unicode_key": (65564, 3), "max_count": (81935, 2), "bs8_empty": (60, 5)}
    for name, (data_len, nblocks) in want.items():
        assert (by[name]["meta_block_offset"], len(by[name]["meta_blocks"])) == (data_len, nblocks), name
    assert by["full_4096x16"]["meta_blocks"][1]["offset"] == 65536 + 2 * 4096 + 2  # block 0: 65536 data bytes
    assert by["one_under_full"]["meta_blocks"][1]["offset"] == 65535 + 2 * 4096 + 2
    assert by["max_count"]["meta_blocks"][1]["offset"] == 81922  # 8192 records: the most a block encodes to
    big = by["big_unicode_key"]["meta_blocks"][1]["first_key"]
    assert (big["chars"], big["bytes"]) == (16382, 65522)
    # utf8_mix: every key start / end offset mod 16, and a continuation byte at every residue
    keys = by["utf8_mix"]["_keys"]
    starts, ends, conts, at = set(), set(), set(), 0
    for k in keys:
        b = k.encode("utf-8")
        starts.add(at % 16)
        ends.add((at + len(b)) % 16)
        conts.update((at + j) % 16 for j, ch in enumerate(b) if ch & 0xC0 == 0x80)
        at += len(b)
    assert starts == ends == conts == set(range(16))
    assert {len(k) for k in keys} == set(range(41))
    assert {len(ch.encode()) for k in keys for ch in k} == {1, 2, 3, 4}
    assert any(k and all(ord(ch) > 127 for ch in k) for k in keys)  # a key of multi-byte characters only


@pytest.mark.parametrize("case", SST_CASES, ids=SST_IDS)
def test_oracle_matches_reference_edge_file(oracle, case):
    keys, vals, bs = case["_keys"], case["_vals"], case["block_size"]
    nb, k = sizing(len(keys), 0.001)
    f = so.sstable_file(keys, vals, bs, oracle.build(nb, k, PackedKeys.from_strs(keys)), k)
    assert len(f) == case["file_len"]
    assert hashlib.sha256(f).hexdigest() == case["file_sha256"]
    data, _, metas = so.data_and_meta(keys, vals, bs)
    assert len(data) == case["meta_block_offset"]
    assert [(key_entry(a), key_entry(b), o) for a, b, o in metas] == golden_metas(case)


@pytest.mark.parametrize("planner", [plan_blocks, plan_blocks_native], ids=["numpy", "native"])
@pytest.mark.parametrize("case", SST_CASES, ids=SST_IDS)
def test_planners_match_reference_edge_file(case, planner):
    keys, vals, bs = case["_keys"], case["_vals"], case["block_size"]
    pk = PackedKeys.from_strs(keys)
    _, vo = pack_values(vals)
    bf, bo = planner(np.asarray(key_offsets(pk), np.uint64), vo, bs)
    assert [int(x) for x in bo[:-1]] == [m["offset"] for m in case["meta_blocks"]]
    assert int(bo[-1]) == case["meta_block_offset"]
    meta, metas = meta_blocks(keys, bf, bo)
    assert [(key_entry(a), key_entry(b), o) for a, b, o in metas] == golden_metas(case)
    assert meta == so.data_and_meta(keys, vals, bs)[1]


@pytest.mark.parametrize("planner", [plan_compaction, plan_compaction_native], ids=["numpy", "native"])
@pytest.mark.parametrize("case", COMPACTION_CASES, ids=COMPACTION_IDS)
def test_compaction_planners_match_reference_edges(case, planner):
    keys, vals = case_records(case)
    pk = PackedKeys.from_strs(keys)
    _, vo = pack_values(vals)
    bf, bo, tb, written = planner(np.asarray(key_offsets(pk), np.uint64), vo, case["block_size"], case["max_sstable_size"])
    outs = case["outputs"]
    assert len(tb) - 1 == len(outs)
    assert written == case["records_written"]
    for t, o in enumerate(outs):
        b0, b1 = int(tb[t]), int(tb[t + 1])
        assert (int(bf[b0]), int(bf[b1])) == (o["first_record"], o["end_record"]), t
        assert int(bo[b1] - bo[b0]) == o["data_len"], t


def test_compaction_edge_cases_are_the_listed_ones():
    by = {c["name"]: c for c in COMPACTION_CASES}
    want = {"split_every_block": (40, 200), "ends_on_closing_block": (1, 17), "ends_on_split": (1, 17),
            "one_after_split": (2, 22), "one_record_blocks": (9, 50), "full_64k_blocks": (1, 8193)}
    for name, (tables, written) in want.items():
        assert (len(by[name]["outputs"]), by[name]["records_written"]) == (tables, written), name


@pytest.mark.parametrize("case", COMPACTION_CASES, ids=COMPACTION_IDS)
def test_oracle_files_match_reference_compaction_edges(oracle, case):
    keys, vals = case_records(case)
    for o in case["outputs"]:
        ks, vs = keys[o["first_record"]:o["end_record"]], vals[o["first_record"]:o["end_record"]]
        nb, k = sizing(len(ks), 0.001)
        assert (nb, k) == (o["nb_bytes"], o["k"])
        f = so.sstable_file(ks, vs, case["block_size"], oracle.build(nb, k, PackedKeys.from_strs(ks)), k)
        assert len(f) == o["file_len"] and hashlib.sha256(f).hexdigest() == o["file_sha256"]


def test_build_entry_points_refuse_bad_arguments():
    """The Python-level refusals of build_sstable / build_sstables, all raised before any device
    work.  (An empty run is not an error for build_sstables: compaction of nothing writes
    nothing, as in the reference.)"""
    from pebbledb_amd.keys import PackedRecords
    from pebbledb_amd.sstable_data import build_sstable, build_sstables
    pr = PackedRecords.from_iter([("a", b"1"), ("b", b"2")])
    for build in (build_sstable, build_sstables):
        with pytest.raises(ValueError, match="differ in length"):
            build(["a", "b"], [b"1"])
        with pytest.raises(ValueError, match="carries its values"):
            build(pr, [b"1", b"2"])
        for bs in (0, 65537):
            with pytest.raises(ValueError, match="block_size must be in"):
                build(["a", "b"], [b"1", b"2"], block_size=bs)
            with pytest.raises(ValueError, match="block_size must be in"):
                build(pr, block_size=bs)
        with pytest.raises(ValueError, match="larger than block_size"):
            build(["a", "b"], [b"1", b"x" * 56], block_size=64)  # 8 + 1 + 56 = 65
    with pytest.raises(ValueError, match="at least one record"):
        build_sstable([], [])
    assert build_sstables([], []) == ([], 0)
