"""tests/memtable_read_model.py pinned to the reference's golden memtable reads
(tests/golden/memtable_read.json, written by tools/gen_golden_memtable_read.py from the REAL
MemTable and LsmStorage), and what of the device memtable's surface needs no device: the
``memtables`` keyword of the three ``lsm_*`` entry points, the refusal of a non-ASCII key at
``put``, and the binding of every new C entry."""
import hashlib
import inspect
import json
import os

import numpy as np
import pytest

import pebbledb_amd
from pebbledb_amd import _native, lsm_get, lsm_scan
from pebbledb_amd.device_memtable import DeviceMemTable, MAX_MEMTABLES
from pebbledb_amd.keys import PackedRecords

import memtable_model as MT
import memtable_read_model as MR
import merge_model as MM

GOLDEN = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "memtable_read.json")))
STORE = GOLDEN["store"]


def sha(parts) -> str:
    return hashlib.sha256(b"".join(parts)).hexdigest()


# ------------------------------------------------------------------ the model against the reference
@pytest.mark.parametrize("case", MT.CASES, ids=[c["name"] for c in MT.CASES])
def test_model_memtable_get_matches_the_reference(case):
    gold = next(g for g in GOLDEN["logs"] if g["name"] == case["name"])
    puts = MT.case_puts(case)
    probes = MR.log_probes(puts)
    m = MR.ModelMemTable(puts)
    assert len(probes) == gold["probes"] and m.approximate_size == gold["approximate_size"]
    digest = MR.probe_digest([m.get(k) for k in probes])
    assert digest == {k: gold[k] for k in digest}
    assert "" in probes and any(p.endswith("\0") for p in probes)


def test_model_store_layout_matches_the_reference():
    assert STORE["rules"] == MR.STORE
    assert STORE["memtable_puts"] == MR.store_memtables()
    layers = MR.store_layers(STORE["level_slices"])
    assert [len(rows) for rows in layers] == STORE["layer_records"]
    assert len(layers) == 6 + len(STORE["level_slices"]) == 6 + len(STORE["level_bounds"])
    for rows, g in zip(layers[:3], STORE["memtable_streams"]):  # the unbounded MemTableIterator of each memtable
        assert (len(rows), sha(k.encode() for k, _ in rows), sha(v for _, v in rows)) == \
            (g["records"], g["keys_sha256"], g["values_sha256"])


def test_model_store_get_matches_the_reference():
    layers = MR.store_layers(STORE["level_slices"])
    probes = MR.store_probes()
    assert len(probes) == STORE["probes"]
    got = MR.get_many(layers, probes)
    runs = []
    for _, u in got:
        if runs and runs[-1][0] == u:
            runs[-1][1] += 1
        else:
            runs.append([u, 1])
    assert runs == STORE["answer_runs"]
    assert MR.probe_digest([v for v, _ in got]) == STORE["get"]
    assert STORE["get"]["empty_hits"] > 100  # empty values answer from the newest holder
    assert {u for _, u in got} == set(range(-1, len(layers)))  # every layer answers somewhere
    assert [MR.get_layers(layers, k) for k in probes[:200]] == got[:200]


def test_model_store_scan_matches_the_reference_after_its_flush():
    layers = MR.store_layers(STORE["level_slices"])[:6]  # LsmStorage.scan: the memtables and level 0
    rngs = MR.ranges_for(layers)
    assert [(n, lo, up) for n, lo, up in rngs] == [(g["name"], g["lower"], g["upper"]) for g in STORE["scans"]]
    for (name, lower, upper), g in zip(rngs, STORE["scans"]):
        run = MR.scan(layers, lower, upper)
        assert len(run) == g["records"], name
        assert (sha(k for k, _, _ in run), sha(v for _, v, _ in run)) == (g["keys_sha256"], g["values_sha256"]), name
        assert MM.source_runs(u for _, _, u in run) == g["source_runs"], name
        assert [hi - lo for lo, hi in MR.windows(layers, lower, upper)] == g["windows"], name
    assert any(g["records"] == 0 for g in STORE["scans"]) and any(g["upper"] == "" for g in STORE["scans"])


def test_the_references_own_memtable_scan_is_short():
    """For the record: the reference's bounded MemTable.scan drops in-range keys."""
    assert GOLDEN["reference_memtable_scan_short_300_keys"] == [899, 900]
    short, total = STORE["reference_memtable_scan_short"]
    assert total == 3 * len(STORE["scans"]) and 0 < short <= total


def test_model_semantics_by_hand():
    m = MR.ModelMemTable([("b", b"1"), ("a", b""), ("b", b"22"), ("a\0", b"3")])
    assert (m.get("b"), m.get("a"), m.get("a\0"), m.get(""), m.get("c")) == (b"22", b"", b"3", None, None)
    assert m.approximate_size == (8 + 1 + 1) + (8 + 1) + (8 + 1 + 2) + (8 + 2 + 1)
    assert m.rows() == [(b"a", b""), (b"a\0", b"3"), (b"b", b"22")]
    assert (m.window("a", "a"), m.window("a\0", ""), m.window("b", "a"), m.window("", "")) == ((0, 1), (1, 3), (2, 2), (0, 3))
    layers = [[("a", b""), ("c", b"new")], [("a", b"old"), ("b", b"x")]]
    assert MR.get_many(layers, ["a", "b", "c", "d"]) == [(b"", 0), (b"x", 1), (b"new", 0), (None, -1)]
    assert MR.scan(layers, "a", "b") == [(b"a", b"", 0), (b"b", b"x", 1)]
    assert MR.lower_bound([b"a", b"a\0", b"b"], "a\0") == (1, True) and MR.lower_bound([b"a"], "b") == (1, False)


# ------------------------------------------------------------------ the surface, without a device
def test_package_exports_the_memtable():
    assert pebbledb_amd.DeviceMemTable is DeviceMemTable and "DeviceMemTable" in pebbledb_amd.__all__
    assert MAX_MEMTABLES == 16


def test_every_new_entry_is_declared_and_bound():
    names = ["pbf_mt_create", "pbf_mt_destroy", "pbf_mt_apply", "pbf_mt_info", "pbf_mt_read", "pbf_mt_get",
             "pbf_mt_gather", "pbf_mt_scan_size", "pbf_mt_scan", "pbf_mt_flush_begin"]
    declared = _native.header_functions()
    for n in names:
        assert n in declared and n in _native.SIGNATURES


def test_memtables_keyword_defaults_to_none_given():
    for fn in (lsm_get.get_batch, lsm_get.get_many, lsm_scan.scan_ranges, lsm_scan.scan_tables, lsm_scan.count_ranges):
        p = inspect.signature(fn).parameters["memtables"]
        assert p.default == () and list(inspect.signature(fn).parameters)[-1] == "memtables"


def test_without_memtables_the_entry_points_answer_as_before():
    """memtables=() takes the paths that stood before the keyword: the same early results, the same
    refusals, no device touched."""
    for kw in ({}, {"memtables": ()}, {"memtables": []}):
        table, vals, offs = lsm_get.get_batch(["a", "b"], [], [], **kw)
        assert table.tolist() == [-1, -1] and table.dtype == np.int32
        assert vals.size == 0 and offs.tolist() == [0, 0, 0] and offs.dtype == np.uint64
        assert lsm_get.get_many(["a", "b"], [], [[]], **kw) == [None, None]
        assert lsm_get.get_many([], [], [], **kw) == []
        for call in (lambda: lsm_scan.scan_ranges([], [("a", "b")], **kw), lambda: lsm_scan.scan_tables([], "a", "b", **kw),
                     lambda: lsm_scan.count_ranges([], [("a", "b")], **kw)):
            with pytest.raises(ValueError, match="no tables to scan"):
                call()
        with pytest.raises(ValueError, match="at most 64 tables"):
            lsm_scan.scan_ranges([None] * 65, [("a", "b")], **kw)


def test_too_many_memtables_are_refused_before_the_device():
    mts = [DeviceMemTable(device=0) for _ in range(17)]
    with pytest.raises(ValueError, match="at most 16 memtables, got 17"):
        lsm_scan.scan_ranges([], [("a", "b")], memtables=mts)
    with pytest.raises(ValueError, match="at most 16 memtables, got 17"):
        lsm_get.get_batch(["a"], [], [], memtables=mts)


def test_put_refuses_a_non_ascii_key_with_flush_logs_wording():
    m = DeviceMemTable(device=0)
    want = "a put log with a non-ASCII key cannot be flushed"
    with pytest.raises(ValueError, match=want):
        m.put("clé", b"v")
    with pytest.raises(ValueError, match=want):
        m.put_many(["ok", "naïve"], [b"1", b"2"])
    with pytest.raises(ValueError, match=want):
        m.put_many(PackedRecords.from_iter([("ok", b"1"), ("ü", b"2")]))
    with pytest.raises(ValueError, match=want):  # the wording is memtable.flush_log's
        pebbledb_amd.memtable._as_log([("ü", b"2")])
    assert m.approximate_size == 0
    m.put("ok", b"12")          # buffered on the host: no device needed
    m.put("ok", b"")            # a re-put counts again (memtable.py:68-72)
    assert m.approximate_size == (8 + 2 + 2) + (8 + 2 + 0)
    with pytest.raises(TypeError):
        m.put(b"bytes-key", b"v")


def test_closed_memtable_refuses_puts_without_a_device():
    m = DeviceMemTable(device=0)
    m.put("a", b"1")
    m.close()
    m.close()
    for call in (lambda: m.put("b", b"2"), lambda: m.sync(), lambda: m.get("a"), lambda: len(m),
                 lambda: m.put_many([("b", b"2")]), lambda: m.records(), lambda: m.scan("", ""),
                 lambda: m.flush_resident(), lambda: m.flush()):
        with pytest.raises(ValueError, match="the memtable is closed"):
            call()
