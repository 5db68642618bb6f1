"""tests/scan_model.py (the GPU scan tests' oracle) pinned to the REAL reference's bounded scans
(tests/golden/lsm_scan.json, tools/gen_golden_scan.py: SSTableBuilder, SSTable.scan,
MergingIterator, and one case through LsmStorage.scan): per range the record count, the key and
value stream hashes, the per-record source table and every table's own window size."""
import ctypes
import json
import os
import re

import pytest

from pebbledb_amd import _native, lsm_scan

import merge_model as MM
import scan_model as SM

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "lsm_scan.json")
CASES = json.load(open(GOLDEN, encoding="utf-8"))["cases"]
IDS = [c["name"] for c in CASES]
WANTED = {"both_stored", "both_absent", "bounds_in_some_tables", "lower_eq_upper_stored", "lower_eq_upper_absent",
          "inverted", "from_start", "to_end", "everything", "below_all", "above_all", "prefix_bounds",
          "extended_bounds", "non_ascii_bounds"}


def test_golden_holds_the_models_cases_and_ranges():
    """The fixture was generated from the rules the model states now, and holds every kind of
    range the scan must get right."""
    keys = ("name", "key", "vlen", "empty", "tables", "table_block_size")
    assert [{k: c[k] for k in keys} for c in CASES] == [{k: c[k] for k in keys} for c in SM.CASES]
    assert tuple(IDS) == SM.CASE_NAMES
    for c in CASES:
        assert [(r["name"], r["lower"], r["upper"]) for r in c["ranges"]] == SM.case_ranges(c)
        names = {r["name"] for r in c["ranges"]}
        # (every_table stores every key in every table: no bound is held by some tables only)
        assert names >= (WANTED - {"bounds_in_some_tables"} if c["name"] == "every_table" else
                         WANTED | {"lower_in_tables_0_and_2"}), c["name"]
        assert max(c["blocks"]) < 300  # far from the reference's recursion limit
    assert [c["name"] for c in CASES if c["via_lsm_storage"]] == [SM.LSM_CASE]


def test_the_ranges_are_the_kinds_their_names_state():
    for c in CASES:
        tables = MM.case_tables(c)
        sets = [{k for k, _ in rows} for rows in tables]
        union = set().union(*sets)
        r = {x["name"]: x for x in c["ranges"]}
        assert r["both_stored"]["lower"] in union and r["both_stored"]["upper"] in union
        assert r["both_absent"]["lower"] not in union and r["both_absent"]["upper"] not in union
        assert r["both_absent"]["records"] > 0
        k = r["lower_eq_upper_stored"]
        assert k["lower"] == k["upper"] and k["lower"] in union and k["records"] == 1
        k = r["lower_eq_upper_absent"]
        assert k["lower"] == k["upper"] and k["lower"] not in union and k["records"] == 0
        assert r["inverted"]["lower"] > r["inverted"]["upper"] and r["inverted"]["records"] == 0
        assert r["below_all"]["records"] == r["above_all"]["records"] == r["non_ascii_lower_only"]["records"] == 0
        assert r["everything"]["records"] == len(union)
        assert r["from_start"]["records"] + r["to_end"]["records"] == len(union) + 1  # both hold the bound
        p = r["prefix_bounds"]
        assert any(x.startswith(p["lower"]) and x != p["lower"] for x in union) and p["lower"] not in union
        e = r["extended_bounds"]
        assert e["lower"][:-1] in union and e["upper"][:-1] in union and e["records"] > 0
        assert not r["non_ascii_bounds"]["lower"].isascii() and r["non_ascii_bounds"]["records"] > 0
        if "lower_in_tables_0_and_2" in r:
            lo = r["lower_in_tables_0_and_2"]["lower"]
            assert lo in sets[0] and lo in sets[2] and lo not in sets[1]
            assert r["lower_in_tables_0_and_2"]["source_runs"][0][0] == 0  # table 0's copy leads the run


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_model_scan_matches_reference(case):
    tables = MM.case_tables(case)
    for r in case["ranges"]:
        run = SM.scan(tables, r["lower"], r["upper"])
        assert len(run) == r["records"], r["name"]
        assert MM.stream_hashes(run) == (r["keys_sha256"], r["values_sha256"]), r["name"]
        assert MM.source_runs(t for _, _, t in run) == r["source_runs"], r["name"]
        assert [hi - lo for lo, hi in SM.windows(tables, r["lower"], r["upper"])] == r["table_records"], r["name"]
        assert SM.presum(tables, r["lower"], r["upper"])[0] == sum(r["table_records"])
        for t, rows in enumerate(tables):
            assert len(SM.scan_one(rows, r["lower"], r["upper"])) == r["table_records"][t]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_open_scan_is_the_merge_of_the_whole_tables(case):
    tables = MM.case_tables(case)
    assert SM.scan(tables, "", "") == MM.merge(tables)
    assert [SM.window(rows, "", "") for rows in tables] == [(0, len(rows)) for rows in tables]


def test_model_semantics_by_hand():
    """Inclusive at both ends; "" as upper is open, as lower it is the start; the lowest table
    index wins inside the range; a key outside a table's window does not shadow anything."""
    t0 = [("b", b"0"), ("d", b"")]
    t1 = [("a", b"1"), ("b", b"1"), ("c", b"1")]
    t2 = [("c", b"2"), ("d", b"2"), ("e", b"2")]
    ts = [t0, t1, t2]
    assert SM.scan(ts, "b", "d") == [(b"b", b"0", 0), (b"c", b"1", 1), (b"d", b"", 0)]
    assert SM.scan(ts, "c", "") == [(b"c", b"1", 1), (b"d", b"", 0), (b"e", b"2", 2)]
    assert SM.scan(ts, "", "a") == [(b"a", b"1", 1)]
    assert SM.scan(ts, "d", "b") == [] and SM.scan(ts, "bb", "bc") == []
    assert SM.windows(ts, "b", "d") == [(0, 2), (1, 3), (0, 2)]
    assert SM.windows(ts, "d", "b") == [(1, 1), (3, 3), (1, 1)]
    assert SM.presum(ts, "b", "d") == (6, 6, 5)
    assert SM.scan_one(t2, "cc", "e") == [(b"d", b"2"), (b"e", b"2")]
    assert SM.window([(b"\x7f", b""), (b"\xc3\xa9", b"")], "é", "é") == (1, 2)  # a str bound is its UTF-8 bytes


def test_scan_constants_and_refusals_need_no_gpu():
    """The segment cap is the header's; the argument checks that come before any device call
    answer without a GPU, and the Python layer refuses what the reference would misread."""
    text = open(_native.HEADER).read()
    assert (1 << int(re.search(r"#define\s+PBF_SCAN_MAX_SEGMENTS\s+\(1ull\s*<<\s*(\d+)\)", text).group(1))
            == lsm_scan.MAX_SEGMENTS == 1 << 22)
    L = _native.lib()
    z = ctypes.c_uint64()
    hs = (ctypes.c_void_p * 65)()
    bounds = (None, None, None, None, None, 0)
    size_tail = (None, None, ctypes.byref(z), ctypes.byref(z), ctypes.byref(z))
    scan_tail = (None, 0, None, None, 0, None, 0, ctypes.byref(z), ctypes.byref(z), ctypes.byref(z), None, 0, None)
    assert L.pbf_sst_scan_size(hs, 0, *bounds, *size_tail) == _native.PBF_ERR_INVALID and b"no tables" in L.pbf_last_error()
    assert L.pbf_sst_scan(hs, 0, *bounds, *scan_tail) == _native.PBF_ERR_INVALID and b"no tables" in L.pbf_last_error()
    assert L.pbf_sst_scan_size(hs, 65, *bounds, *size_tail) == _native.PBF_ERR_INVALID and b"at most 64" in L.pbf_last_error()
    assert L.pbf_sst_scan(hs, 65, *bounds, *scan_tail) == _native.PBF_ERR_INVALID and b"at most 64" in L.pbf_last_error()
    assert L.pbf_sst_scan(hs, 2, *bounds, *scan_tail) == _native.PBF_ERR_INVALID and b"listed twice" in L.pbf_last_error()
    big = (None, None, None, None, None, (1 << 22) // 3 + 1)
    hs3 = (ctypes.c_void_p * 3)(1, 2, 3)  # (never dereferenced: the cap is checked first)
    assert L.pbf_sst_scan(hs3, 3, *big, *scan_tail) == _native.PBF_ERR_INVALID and b"ranges x tables" in L.pbf_last_error()
    with pytest.raises(ValueError, match="no tables"):
        lsm_scan.scan_tables([], "a", "b")
    with pytest.raises(ValueError, match="no tables"):
        lsm_scan.scan_ranges([], [("a", "b")])
    with pytest.raises(ValueError, match="no tables"):
        lsm_scan.count_ranges([], [("a", "b")])
    for bad in ((None, "b"), ("a", None), (None, None), (b"a", "b")):
        with pytest.raises(ValueError, match=r"records\(\) / merge_tables"):
            lsm_scan._Bounds([bad])
    b = lsm_scan._Bounds([("a", ""), ("é", "zz")])
    assert b.open.tolist() == [1, 0] and b.lower_offsets.tolist() == [0, 1, 3] and b.upper_offsets.tolist() == [0, 0, 2]
    assert b.lower.tobytes() == "aé".encode()
