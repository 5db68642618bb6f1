"""The resident write path end to end: ``compact_l0_resident`` / ``compact_level_resident`` and
``flush_log_resident`` / ``flush_wal_resident`` against the reference's golden files and, on
other shapes, byte for byte against the host-round-trip path (``compact_l0`` / ``compact_level`` /
``flush_log``); the outputs as tables (meta blocks, get_many, scan, records()); the chain flush ->
compaction -> reads -> compaction with nothing but resident tables; and the refusals, which leave
the library usable and hold no memory."""
import ctypes
import hashlib
import json
import os
import struct

import numpy as np
import pytest

from pebbledb_amd import DeviceSSTable, _native, compaction, memtable
from pebbledb_amd.bloom_filter import BloomFilter
from pebbledb_amd.compaction import (compact_l0, compact_l0_resident, compact_level, compact_level_resident)
from pebbledb_amd.keys import PackedRecords
from pebbledb_amd.lsm_get import get_batch
from pebbledb_amd.lsm_scan import scan_tables
from pebbledb_amd.memtable import flush_log, flush_log_resident, flush_wal_resident
from pebbledb_amd.sstable_data import build_sstable, filter_sizing

import memtable_model as MT
import merge_model as MM

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

vp = ctypes.c_void_p
HERE = os.path.dirname(__file__)
MERGE_CASES = json.load(open(os.path.join(HERE, "golden", "compaction_merge.json")))["cases"]
FLUSH_CASES = json.load(open(os.path.join(HERE, "golden", "memtable_flush.json")))["cases"]


@pytest.fixture
def opened():
    """opened(rows, block_size) builds a table from (str key, value) rows and opens it; opened.keep(t)
    adopts a table made elsewhere.  Everything is closed afterwards (close() twice is fine)."""
    handles = []

    def _open(rows, block_size=256):
        f, _, _ = build_sstable([k for k, _ in rows], [v for _, v in rows], block_size)
        handles.append(DeviceSSTable.from_bytes(f))
        return handles[-1]

    def _keep(tables):
        handles.extend(tables)
        return tables

    _open.keep = _keep
    yield _open
    for t in handles:
        t.close()


def records_of(pr):
    kb, vb = pr.keys.data.tobytes(), np.asarray(pr.values).tobytes()
    ko, vo = pr.keys.offsets, pr.value_offsets
    return [(kb[int(ko[i]):int(ko[i + 1])], vb[int(vo[i]):int(vo[i + 1])]) for i in range(pr.n)]


def sha(a) -> str:
    return hashlib.sha256(bytes(a)).hexdigest()


def value(tag: int, i: int, n: int = None) -> bytes:
    return MM.value_of(tag * 1000 + i, 1 + (tag * 5 + i) % 23 if n is None else n)


def rows_of(tag: int, idx, key="k{i:05d}"):
    return [(key.format(i=i), value(tag, i)) for i in idx]


def check_table(t, part, ordered=True):
    """An output against its slice of the model's run, [(key bytes, value)]: the attributes
    from_bytes sets, then records(), get_many and scan."""
    assert (t.nrecords, t.first_key, t.last_key) == (len(part), part[0][0].decode(), part[-1][0].decode())
    assert t.nblocks == len(t.meta_blocks) and t.meta_block_offset == t.data_len
    assert t.meta_blocks[0][2] == 0 and (t.meta_blocks[0][0], t.meta_blocks[-1][1]) == (t.first_key, t.last_key)
    assert isinstance(t.bloom_filter, BloomFilter)
    assert (t.bloom_filter.nb_bytes, t.bloom_filter.nb_hash_functions) == filter_sizing(len(part), 0.001)
    if not ordered:
        return
    assert records_of(t.records()) == part
    keys = [k.decode() for k, _ in part]
    found, values, offs = t.get_many(keys + ["zz-absent", "0-absent"])
    raw = values.tobytes()
    assert found[:-2].all() and not found[-2:].any()
    assert [raw[int(offs[i]):int(offs[i + 1])] for i in range(len(part))] == [v for _, v in part]
    lo, hi = keys[len(keys) // 4], keys[(3 * len(keys)) // 4]
    assert records_of(t.scan(lo, hi)) == [r for r in part if lo.encode() <= r[0] <= hi.encode()]
    assert all(t.bloom_filter.may_contain(k) for k in keys[:: max(1, len(keys) // 16)])


def check_against_host(tables, mode, max_sstable_size, block_size, rows, opened):
    """compact_*_resident over the open tables against compact_* byte for byte (each file, each
    filter) and against the model's run; returns the resident outputs."""
    host_fn, res_fn = (compact_l0, compact_l0_resident) if mode == "merge" else (compact_level, compact_level_resident)
    outs, written = host_fn(tables, max_sstable_size=max_sstable_size, block_size=block_size)
    res, res_written = res_fn(tables, max_sstable_size=max_sstable_size, block_size=block_size)
    opened.keep(res)
    assert (len(res), res_written) == (len(outs), written)
    run = [(k, v) for k, v, _ in MM.run_of(rows, mode)]
    at = 0
    for t, (f, metas, bloom) in zip(res, outs):
        assert bytes(t.to_bytes()) == bytes(f)
        assert t.bloom_filter == bloom
        assert t.meta_blocks == metas
        part = run[at:at + t.nrecords]
        at += t.nrecords
        check_table(t, part, ordered=all(a[0] < b[0] for a, b in zip(part, part[1:])))
    assert at == written
    return res


# ------------------------------------------------------------------ the reference's golden files
@pytest.mark.parametrize("case", MERGE_CASES, ids=[c["name"] for c in MERGE_CASES])
def test_golden_compaction(opened, case):
    rows = MM.case_tables(case)
    tables = [opened(r, case["table_block_size"]) for r in rows]
    fn = compact_l0_resident if case["mode"] == "merge" else compact_level_resident
    res, written = fn(tables, max_sstable_size=case["max_sstable_size"], block_size=case["block_size"])
    opened.keep(res)
    assert written == case["records_written"] and len(res) == len(case["outputs"])
    run = [(k, v) for k, v, _ in MM.run_of(rows, case["mode"])]
    at = 0
    for t, o in zip(res, case["outputs"]):
        f = t.to_bytes()
        assert (len(f), sha(f)) == (o["file_len"], o["file_sha256"])
        assert (t.first_key, t.last_key) == (o["first_key"], o["last_key"])
        part = run[at:at + t.nrecords]
        at += t.nrecords
        check_table(t, part, ordered=all(a[0] < b[0] for a, b in zip(part, part[1:])))
    assert at == written


@pytest.mark.parametrize("case", FLUSH_CASES, ids=[c["name"] for c in FLUSH_CASES])
def test_golden_flush(opened, case, tmp_path):
    puts = MT.case_puts(case)
    t = flush_log_resident(puts, block_size=case["block_size"])
    opened.keep([t])
    f = t.to_bytes()
    assert (len(f), sha(f)) == (case["sst_len"], case["sst_sha256"])
    check_table(t, [(r[0], r[1]) for r in MT.flush_run(puts)])
    wal = MT.wal_bytes(puts)
    u = flush_wal_resident(wal, block_size=case["block_size"])
    opened.keep([u])
    assert sha(u.to_bytes()) == case["sst_sha256"]
    path = tmp_path / "memtable.wal"
    path.write_bytes(wal)
    v = flush_wal_resident(str(path), block_size=case["block_size"])
    opened.keep([v])
    out = tmp_path / "out.sst"
    v.write(out)
    assert sha(out.read_bytes()) == case["sst_sha256"]


# ------------------------------------------------------------------ other shapes, against the host path
def test_one_table(opened):
    rows = [rows_of(1, range(700))]
    tables = [opened(rows[0], 512)]
    assert len(check_against_host(tables, "merge", 4096, 1024, rows, opened)) > 1
    assert len(check_against_host(tables, "concat", 1 << 20, 1024, rows, opened)) == 1
    assert check_against_host(tables, "concat", 1 << 20, 65_536, rows, opened) == []


def test_sixty_four_tables(opened):
    rows = [rows_of(t, range(t % 7, 900, 5 + t % 11)) for t in range(64)]
    tables = [opened(r, 300) for r in rows]
    check_against_host(tables, "merge", 6000, 1024, rows, opened)


def test_shadowed_table_and_empty_values(opened):
    rows = [[(f"k{i:05d}", b"" if i % 3 == 0 else value(1, i)) for i in range(100, 700)],
            rows_of(2, range(200, 500)),
            [(f"k{i:05d}", b"") for i in range(0, 900, 7)]]
    tables = [opened(r, 400) for r in rows]
    check_against_host(tables, "merge", 5000, 512, rows, opened)
    only_empty = [[(f"e{i:04d}", b"") for i in range(0, 500, 2)], [(f"e{i:04d}", b"") for i in range(1, 500, 2)]]
    tables = [opened(r, 128) for r in only_empty]
    check_against_host(tables, "merge", 900, 128, only_empty, opened)


def test_concat_out_of_order(opened):
    """Tables out of key order under concat: the outputs are the files _compact writes (their keys
    do not ascend across the seam), byte for byte."""
    rows = [rows_of(1, range(1000, 1500)), rows_of(2, range(0, 400)), rows_of(3, range(500, 900, 2))]
    tables = [opened(r, 512) for r in rows]
    check_against_host(tables, "concat", 8192, 1024, rows, opened)


def test_several_outputs_with_a_dropped_tail(opened):
    case = next(c for c in MERGE_CASES if c["name"] == "multi_output_tail_dropped")
    rows = MM.case_tables(case)
    tables = [opened(r, 1024) for r in rows]
    res = check_against_host(tables, "merge", case["max_sstable_size"], case["block_size"], rows, opened)
    assert sum(t.nrecords for t in res) < len(MM.merge(rows)) and len(res) > 2


def test_forty_outputs(opened):
    """More outputs than the filter stream pool has streams: the builds go round it."""
    rows = [rows_of(1, range(0, 6000, 2)), rows_of(2, range(1, 6000, 2))]
    tables = [opened(r, 1024) for r in rows]
    res = check_against_host(tables, "merge", 2500, 512, rows, opened)
    assert len(res) >= 40


def test_no_output(opened):
    rows = [rows_of(1, range(5))]
    res, written = compact_l0_resident([opened(rows[0])], max_sstable_size=100, block_size=4096)
    assert (res, written) == ([], 0)


def test_flush_spanning_sort_tiles_and_merge_passes(opened):
    """40000 puts: 20 sort tiles and two merge passes; with duplicates, empty values and keys of
    several lengths."""
    n = 40_000
    assert memtable.merge_passes(n) == 2
    puts = [(f"key{MT.mix(3, i) % 30_000:07d}" + "x" * (i % 3), b"" if i % 11 == 0 else MT.value_of(i, 1 + i % 40))
            for i in range(n)]
    log = PackedRecords.from_iter(puts)
    f, metas, bloom = flush_log(log, block_size=4096)
    t = flush_log_resident(log, block_size=4096)
    opened.keep([t])
    assert bytes(t.to_bytes()) == bytes(f) and t.bloom_filter == bloom and t.meta_blocks == metas
    check_table(t, [(r[0], r[1]) for r in MT.flush_run(puts)])


# ------------------------------------------------------------------ the chain
def test_flush_compact_read_compact_chain(opened):
    """Three logs flushed resident, compacted resident with the inputs closed before the outputs
    are read, get_batch and scan_tables over the outputs against a newest-wins dict, and the
    outputs fed to a second resident compaction."""
    logs, model = [], {}
    for g in range(3):  # g = 2 is the newest
        puts = [(f"u{MT.mix(g + 5, i) % 5000:05d}", b"" if (i + g) % 13 == 0 else MT.value_of(g * 100_000 + i, 1 + i % 30))
                for i in range(4000)]
        logs.append(puts)
        for k, v in puts:
            model[k] = v
    flushed = [flush_log_resident(p, block_size=1024) for p in logs]
    opened.keep(flushed)
    newest_first = flushed[::-1]
    outs, written = compact_l0_resident(newest_first, max_sstable_size=30_000, block_size=2048)
    opened.keep(outs)
    for t in flushed:
        t.close()
    run = sorted((k.encode(), v) for k, v in model.items())
    assert len(outs) > 2 and written <= len(run)
    kept = run[:written]
    assert [r for t in outs for r in records_of(t.records())] == kept
    probe = [k.decode() for k, _ in run[::3]] + ["u99999", "a"]
    table, vals, offs = get_batch(probe, [], [outs])
    raw, have = vals.tobytes(), dict(kept)
    for i, k in enumerate(probe):
        want = have.get(k.encode())
        assert (table[i] >= 0) == (want is not None), k
        if want is not None:
            assert raw[int(offs[i]):int(offs[i + 1])] == want, k
    lo, hi = "u01000", "u03500"
    assert records_of(scan_tables(outs, lo, hi)) == [r for r in kept if lo.encode() <= r[0] <= hi.encode()]
    again, written2 = compact_level_resident(outs, max_sstable_size=1 << 20, block_size=4096)
    opened.keep(again)
    host, host_written = compact_level(outs, max_sstable_size=1 << 20, block_size=4096)
    assert written2 == host_written and [bytes(t.to_bytes()) for t in again] == [bytes(f) for f, _, _ in host]
    assert [r for t in again for r in records_of(t.records())] == kept[:written2]


def test_to_bytes_of_a_table_opened_from_bytes(opened):
    rows = rows_of(4, range(1500))
    f, _, _ = build_sstable([k for k, _ in rows], [v for _, v in rows], 512)
    t = DeviceSSTable.from_bytes(f)
    opened.keep([t])
    assert bytes(t.to_bytes()) == bytes(f)
    t.close()
    with pytest.raises(ValueError, match="closed"):
        t.to_bytes()


# ------------------------------------------------------------------ refusals
def _scratch_after_trim() -> int:
    out = ctypes.c_uint64()
    _native.check(_native.lib().pbf_trim(0), "pbf_trim")
    _native.check(_native.lib().pbf_scratch_bytes(0, ctypes.byref(out)), "pbf_scratch_bytes")
    return out.value


def _begin(tables, mode=_native.PBF_MERGE_DEDUP, block_size=1024, max_sstable_size=4096):
    hs = (vp * len(tables))(*[t.handle.value for t in tables])
    job, nt, w = vp(), ctypes.c_uint64(), ctypes.c_uint64()
    rc = _native.lib().pbf_compact_begin(hs, len(tables), mode, block_size, max_sstable_size, ctypes.byref(job),
                                         ctypes.byref(nt), ctypes.byref(w))
    return rc, job, nt.value, w.value


def test_refusals_leave_the_library_usable_and_hold_nothing(opened):
    lib = _native.lib()
    rows = [rows_of(1, range(0, 600, 2)), rows_of(2, range(1, 600, 2))]
    tables = [opened(r, 512) for r in rows]
    before = [records_of(t.records()) for t in tables]
    base = _scratch_after_trim()
    err = lambda: lib.pbf_last_error().decode()  # noqa: E731

    # a closed handle, and a handle listed twice
    gone = opened(rows_of(3, range(50)))
    gone.close()
    with pytest.raises(ValueError, match="closed"):
        compact_l0_resident([tables[0], gone])
    hs = (vp * 2)(tables[0].handle.value, tables[0].handle.value)
    job, nt, w = vp(), ctypes.c_uint64(), ctypes.c_uint64()
    rc = lib.pbf_compact_begin(hs, 2, 0, 1024, 4096, ctypes.byref(job), ctypes.byref(nt), ctypes.byref(w))
    assert rc == _native.PBF_ERR_INVALID and "listed twice" in err() and not job.value
    rc = lib.pbf_compact_begin(hs, 1, 7, 1024, 4096, ctypes.byref(job), ctypes.byref(nt), ctypes.byref(w))
    assert rc == _native.PBF_ERR_INVALID and "merge mode" in err() and not job.value

    # a record over block_size in begin: compaction and flush
    big = opened([("big", b"v" * 300), ("bih", b"w")], 512)
    with pytest.raises(ValueError, match="a record is larger than block_size"):
        compact_l0_resident([big, tables[0]], block_size=128)
    with pytest.raises(ValueError, match="a record is larger than block_size"):
        flush_log_resident([("a", b"1"), ("b", b"x" * 200)], block_size=64)

    # abort after begin; the handle is then refused everywhere
    rc, job, nt, _ = _begin(tables)
    assert rc == 0 and nt > 1
    assert lib.pbf_job_abort(job) == 0
    assert lib.pbf_job_abort(job) == _native.PBF_ERR_INVALID
    assert lib.pbf_job_table_info(job, 0, None, None, None, None) == _native.PBF_ERR_INVALID
    assert lib.pbf_job_finish(job, None, None, None, None, None) == _native.PBF_ERR_INVALID and "job handle" in err()

    # finish with a filter missing, and with one listed twice: the job is gone either way
    for make in (lambda fs: [fs[0].handle.value] + [None] * (len(fs) - 1),
                 lambda fs: [fs[0].handle.value] * len(fs)):
        rc, job, nt, _ = _begin(tables)
        assert rc == 0
        nr = ctypes.c_uint64()
        filters = []
        for t in range(nt):
            assert lib.pbf_job_table_info(job, t, ctypes.byref(nr), None, None, None) == 0
            filters.append(BloomFilter(*filter_sizing(nr.value, 0.001)))
        hs = (vp * nt)(*make(filters))
        sink = np.zeros(1 << 16, np.uint8)
        handles = (vp * nt)()
        rc = lib.pbf_job_finish(job, hs, vp(sink.ctypes.data), vp(sink.ctypes.data), vp(sink.ctypes.data), handles)
        assert rc == _native.PBF_ERR_INVALID and ("null filter" in err() or "twice" in err())
        assert not any(handles)
        assert lib.pbf_job_abort(job) == _native.PBF_ERR_INVALID

    # nothing is held, the inputs are untouched, and the next compaction gives the right bytes
    assert _scratch_after_trim() == base
    assert [records_of(t.records()) for t in tables] == before
    check_against_host(tables, "merge", 4096, 1024, rows, opened)
    assert _scratch_after_trim() == base


def test_refuses_tables_and_filters_on_two_devices(opened):
    if _native.device_count() < 2:
        pytest.skip("needs two devices")
    rows = rows_of(1, range(300))
    f, _, _ = build_sstable([k for k, _ in rows], [v for _, v in rows], 512)
    a, b = DeviceSSTable.from_bytes(f, device=0), DeviceSSTable.from_bytes(f, device=1)
    opened.keep([a, b])
    with pytest.raises(ValueError, match="share a device"):
        compact_l0_resident([a, b])
    lib = _native.lib()
    rc, job, nt, _ = _begin([a], max_sstable_size=1 << 20)
    assert rc == 0 and nt == 1
    wrong = BloomFilter(*filter_sizing(300, 0.001), device=1)
    sink = np.zeros(1 << 16, np.uint8)
    handles = (vp * 1)()
    rc = lib.pbf_job_finish(job, (vp * 1)(wrong.handle.value), vp(sink.ctypes.data), vp(sink.ctypes.data),
                            vp(sink.ctypes.data), handles)
    assert rc == _native.PBF_ERR_INVALID and "job's device" in lib.pbf_last_error().decode() and not handles[0]


def test_python_refusals(opened):
    t = opened(rows_of(1, range(50)))
    with pytest.raises(struct.error, match="ubyte format"):
        compact_l0_resident([t], max_sstable_size=1 << 20, block_size=256, fp_rate=1e-120)
    with pytest.raises(struct.error, match="ubyte format"):
        flush_log_resident([("a", b"1")], fp_rate=1e-120)
    with pytest.raises(ValueError, match="at least one record"):
        flush_wal_resident(b"")
    assert records_of(t.records()) == [(k.encode(), v) for k, v in rows_of(1, range(50))]
