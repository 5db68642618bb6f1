"""tests/merge_model.py (the GPU merge tests' oracle) pinned to the REAL reference's compaction
runs (tests/golden/compaction_merge.json, tools/gen_golden_merge.py: SSTableBuilder,
SSTableIterator, MergingIterator / ConcatenatingIterator, LsmStorage._compact): the run's record
count, key and value stream hashes and per-record source table; and — through the host planner,
the oracle restatement of the SSTable encoding and the C bloom oracle, as
tests/test_compaction_cpu.py — every output file's length and sha256."""
import hashlib
import json
import os

import numpy as np
import pytest

from oracle import sstable_oracle as so
from oracle.oracle import sizing
from pebbledb_amd import _native, compaction
from pebbledb_amd.keys import PackedKeys
from pebbledb_amd.sstable_data import key_offsets, pack_values, plan_compaction

import merge_model as MM

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "compaction_merge.json")
CASES = json.load(open(GOLDEN))["cases"]
IDS = [c["name"] for c in CASES]


def test_golden_holds_the_models_cases():
    """The fixture was generated from the rules the model states now."""
    keys = ("name", "mode", "key", "vlen", "empty", "tables", "table_block_size", "block_size", "max_sstable_size")
    assert [{k: c[k] for k in keys} for c in CASES] == [{k: c[k] for k in keys} for c in MM.CASES]
    wanted = {"overlap3": 3, "overlap5": 5}
    assert all(len(c["tables"]) == wanted[c["name"]] for c in CASES if c["name"] in wanted)
    assert {c["mode"] for c in CASES} == {"merge", "concat"}


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_model_run_matches_reference(case):
    tables = MM.case_tables(case)
    assert [len(t) for t in tables] == case["input_records"]
    run = MM.run_of(tables, case["mode"])
    assert len(run) == case["records"]
    assert MM.stream_hashes(run) == (case["keys_sha256"], case["values_sha256"])
    assert MM.source_runs(t for _, _, t in run) == case["source_runs"]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_planned_outputs_match_reference(oracle, case):
    """build_sstables' split (plan_compaction) over the model's run gives the reference's output
    files: count, records covered, and each file re-encoded by the oracle restatement."""
    run = MM.run_of(MM.case_tables(case), case["mode"])
    keys, vals = [k.decode() for k, _, _ in run], [v for _, v, _ in run]
    pk = PackedKeys.from_strs(keys)
    _, vo = pack_values(vals)
    bf, _, tb, written = plan_compaction(np.asarray(key_offsets(pk), np.uint64), vo, case["block_size"],
                                         case["max_sstable_size"])
    outs = case["outputs"]
    assert len(tb) - 1 == len(outs) and written == case["records_written"]
    for t, o in enumerate(outs):
        lo, hi = int(bf[int(tb[t])]), int(bf[int(tb[t + 1])])
        ks, vs = keys[lo:hi], vals[lo:hi]
        assert (ks[0], ks[-1]) == (o["first_key"], o["last_key"])
        nb, k = sizing(len(ks), 0.001)
        f = so.sstable_file(ks, vs, case["block_size"], oracle.build(nb, k, PackedKeys.from_strs(ks)), k)
        assert len(f) == o["file_len"] and hashlib.sha256(f).hexdigest() == o["file_sha256"], t


def test_merge_constants_agree_with_the_header_and_refusals_need_no_gpu():
    """The modes and the table limit are the header's and the kernel header's; the argument
    checks that come before any device call answer without a GPU."""
    import ctypes
    import re
    text = open(_native.HEADER).read()
    assert int(re.search(r"#define\s+PBF_MERGE_DEDUP\s+(\d+)", text).group(1)) == _native.PBF_MERGE_DEDUP == 0
    assert int(re.search(r"#define\s+PBF_MERGE_CONCAT\s+(\d+)", text).group(1)) == _native.PBF_MERGE_CONCAT == 1
    kernels = open(os.path.join(os.path.dirname(_native.__file__), "csrc", "sstable_read_kernels.hpp")).read()
    assert int(re.search(r"kSstTablesPerLaunch\s*=\s*(\d+)", kernels).group(1)) == compaction.MAX_TABLES == 64
    L = _native.lib()
    z = ctypes.c_uint64()
    args = (None, 0, None, None, 0, None, 0, ctypes.byref(z), ctypes.byref(z), ctypes.byref(z), 0, None)
    hs = (ctypes.c_void_p * 65)()
    assert L.pbf_sst_merge(hs, 0, 0, *args) == _native.PBF_ERR_INVALID and b"no tables" in L.pbf_last_error()
    assert L.pbf_sst_merge(hs, 65, 0, *args) == _native.PBF_ERR_INVALID and b"at most 64" in L.pbf_last_error()
    with pytest.raises(ValueError, match="no tables"):
        compaction.merge_tables([])


def test_model_semantics_by_hand():
    """The rules in small: the lowest table index wins, an empty value is kept, a key only in
    older tables keeps the NEWEST of those, order is by bytes."""
    t0 = [("b", b"0"), ("d", b"")]
    t1 = [("a", b"1"), ("b", b"1"), ("c", b"1")]
    t2 = [("c", b"2"), ("d", b"2"), ("e", b"2")]
    assert MM.merge([t0, t1, t2]) == [(b"a", b"1", 1), (b"b", b"0", 0), (b"c", b"1", 1), (b"d", b"", 0), (b"e", b"2", 2)]
    assert [t for _, _, t in MM.concat([t2, t0])] == [0, 0, 0, 1, 1]
    assert [k for k, _, _ in MM.merge([[(b"\x80", b"x")], [(b"\x7f", b"y"), (b"\x80\x00", b"z")]])] == \
        [b"\x7f", b"\x80", b"\x80\x00"]
    assert MM.source_runs([0, 0, 2, 2, 2, 0]) == [[0, 2], [2, 3], [0, 1]]
