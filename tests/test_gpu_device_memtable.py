"""The device memtable (pbf_mt_*, csrc/memtable_read_kernels.hpp; pebbledb_amd/device_memtable.py,
the ``memtables`` keyword of lsm_get / lsm_scan): the reference's golden memtable reads end to end,
then every branch of apply, the search, the get stage, the gather, the scan over mixed sources,
the flush and the handle's lifetime at the smallest shapes that enter it.  Expected results come
from tests/memtable_read_model.py and tests/memtable_model.py (pinned to the reference in their
CPU tests); everything is compared bit for bit."""
import ctypes
import hashlib
import itertools
import json
import os
from bisect import bisect_left

import numpy as np
import pytest

from pebbledb_amd import DeviceMemTable, DeviceSSTable, _native, flush_log, lsm_get, sort_log
from pebbledb_amd.device_memtable import _mt_handles, mt_gather, mt_lookup
from pebbledb_amd.keys import PackedKeys, PackedRecords
from pebbledb_amd.lsm_scan import _Bounds, _size, count_ranges, scan_ranges, scan_tables
from pebbledb_amd.sstable_data import build_sstable, key_offsets
from pebbledb_amd.sstable_read import _handles, lookup

import memtable_model as MT
import memtable_read_model as MR
import merge_model as MM
import scan_model as SM

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

vp = ctypes.c_void_p
T = 2048  # the sort tile and the scan tile
GUARD = 0xFF
HERE = os.path.dirname(__file__)
GOLDEN = json.load(open(os.path.join(HERE, "golden", "memtable_read.json"), encoding="utf-8"))
FLUSH = {c["name"]: c for c in json.load(open(os.path.join(HERE, "golden", "memtable_flush.json")))["cases"]}
SCAN_CASES = json.load(open(os.path.join(HERE, "golden", "lsm_scan.json"), encoding="utf-8"))["cases"]
STORE = GOLDEN["store"]


def sha(parts) -> str:
    return hashlib.sha256(b"".join(parts)).hexdigest()


def records_of(pr):
    """[(key bytes, value bytes)] of a PackedRecords."""
    kb, vb = pr.keys.data.tobytes(), np.asarray(pr.values).tobytes()
    ko, vo = key_offsets(pr.keys), pr.value_offsets
    assert len(ko) == len(vo) == pr.n + 1 and ko[0] == 0 and vo[0] == 0
    assert int(ko[-1]) == len(kb) and int(vo[-1]) == len(vb)
    return [(kb[int(ko[i]):int(ko[i + 1])], vb[int(vo[i]):int(vo[i + 1])]) for i in range(pr.n)]


def run_of(puts):
    return [(k, v) for k, v, _ in MT.flush_run(puts)]


@pytest.fixture
def made():
    """Makes memtables and tables and closes what it made: made.mt(puts, ...) applies each put list
    as one batch; made.table(rows, block_size) builds and opens a table."""
    things = []

    class Made:
        @staticmethod
        def mt(*batches):
            m = DeviceMemTable()
            things.append(m)
            for b in batches:
                m.put_many(b)
            return m

        @staticmethod
        def table(rows, block_size=256):
            f, _, _ = build_sstable([k for k, _ in rows], [v for _, v in rows], block_size)
            things.append(DeviceSSTable.from_bytes(f))
            return things[-1]

    yield Made
    for t in things:
        t.close()


def value(i: int, n: int = None) -> bytes:
    return MT.value_of(i, 1 + (i * 5) % 23 if n is None else n)


def raw_keys(keys) -> PackedKeys:
    """Keys given as bytes, packed variable-length (bytes no str encodes to are allowed)."""
    offs = np.zeros(len(keys) + 1, dtype=np.uint64)
    np.cumsum([len(k) for k in keys], out=offs[1:])
    return PackedKeys(np.frombuffer(b"".join(keys) or b"\0", dtype=np.uint8)[:int(offs[-1])], len(keys), offsets=offs)


def check_get(memtables, layers, probes):
    """mt_lookup + mt_gather over host pointers equal the model: source, value and miss mask."""
    pk = probes if isinstance(probes, PackedKeys) else PackedKeys.from_strs(list(probes))
    keys = [pk.key(i) for i in range(pk.n)]
    want = MR.get_many(layers, keys)
    src, vo, vl, miss = mt_lookup(memtables, pk)
    assert src.tolist() == [u for _, u in want]
    assert vl.tolist() == [-1 if v is None else len(v) for v, _ in want]
    bits = np.unpackbits(miss, bitorder="little")
    assert bits[:pk.n].tolist() == [int(v is None) for v, _ in want] and not bits[pk.n:].any()
    vals, offs = mt_gather(memtables, [], np.where(src >= 0, -2 - src, -1), vo, vl)
    raw = vals.tobytes()
    assert [raw[int(offs[i]):int(offs[i + 1])] if src[i] >= 0 else None for i in range(pk.n)] == [v for v, _ in want]
    return want


# ------------------------------------------------------------------ golden: put logs
@pytest.mark.parametrize("case", MT.CASES, ids=[c["name"] for c in MT.CASES])
def test_golden_log_get_records_flush(case, made, tmp_path):
    """The reference's MemTable.get over the golden probe list, the MemTableIterator run, and the
    flush file byte for byte, from puts applied in three batches and from the WAL."""
    gold = next(g for g in GOLDEN["logs"] if g["name"] == case["name"])
    puts = MT.case_puts(case)
    n = len(puts)
    m = made.mt(puts[:n // 3], puts[n // 3:n // 2], puts[n // 2:])
    probes = MR.log_probes(puts)
    got = m.get_many(probes)
    digest = MR.probe_digest(got)
    assert digest == {k: gold[k] for k in digest} and m.approximate_size == gold["approximate_size"]
    model = MR.ModelMemTable(puts)
    assert got == [model.get(k) for k in probes] and m.get(probes[0]) == got[0]
    assert records_of(m.records()) == run_of(puts) and len(m) == FLUSH[case["name"]]["records"]
    want_file = flush_log(puts, block_size=case["block_size"])[0].tobytes()
    assert hashlib.sha256(want_file).hexdigest() == FLUSH[case["name"]]["sst_sha256"]
    table = m.flush_resident(block_size=case["block_size"])
    try:
        assert table.to_bytes().tobytes() == want_file
    finally:
        table.close()
    assert m.flush(block_size=case["block_size"])[0].tobytes() == want_file
    assert records_of(m.records()) == run_of(puts)  # the flush leaves the memtable as it is
    for wal in (MT.wal_bytes(puts), None):
        if wal is None:
            wal = str(tmp_path / "0.wal")
            (tmp_path / "0.wal").write_bytes(MT.wal_bytes(puts))
        w = DeviceMemTable.from_wal(wal)
        try:
            assert records_of(w.records()) == run_of(puts) and w.approximate_size == gold["approximate_size"]
        finally:
            w.close()


# ------------------------------------------------------------------ golden: the store
@pytest.fixture(scope="module")
def store():
    """The golden store on the device: 3 memtables (the puts of their ranges, in put order), 3
    level-0 tables and the level's tables with the bounds the reference gave them."""
    layers = MR.store_layers(STORE["level_slices"])
    ranges = STORE["memtable_puts"]
    mts = []
    for a, b in (ranges[7], ranges[6], ranges[5]):  # active, immutables newest first
        m = DeviceMemTable()
        m.put_many([MR.store_put(p) for p in range(a, b)])
        mts.append(m)
    tables = []
    for rows in layers[3:]:
        f, _, _ = build_sstable([k for k, _ in rows], [v for _, v in rows], STORE["rules"]["block_size"])
        tables.append(DeviceSSTable.from_bytes(f))
    for t, (first, last) in zip(tables[3:], STORE["level_bounds"]):
        t.first_key, t.last_key = first, last  # SSTableBuilder's: its keys list, also of records it did not write
    yield layers, mts, tables
    for x in mts + tables:
        x.close()


def test_golden_store_get(store):
    """get_many(keys, level0, levels, memtables=[active, *immutables]) equals [store.get(k)]."""
    layers, mts, tables = store
    probes = MR.store_probes()
    want = MR.get_many(layers, probes)
    assert MR.probe_digest([v for v, _ in want]) == STORE["get"]
    assert lsm_get.get_many(probes, tables[:3], [tables[3:]], memtables=mts) == [v for v, _ in want]
    table, vals, offs = lsm_get.get_batch(probes, tables[:3], [tables[3:]], memtables=mts)
    assert table.tolist() == [-2 - u if 0 <= u < 3 else (u - 3 if u >= 3 else -1) for _, u in want]
    assert int(offs[-1]) == len(vals) == sum(len(v) for v, _ in want if v)
    # memtables with no tables, and the host-pointer form
    mem_only = MR.get_many(layers[:3], probes)
    assert lsm_get.get_many(probes, [], [], memtables=mts) == [v for v, _ in mem_only]
    check_get(mts, layers[:3], probes)
    # memtables=() is the walk over tables alone
    assert lsm_get.get_many(probes[:500], tables[:3], [tables[3:]]) == [v for v, _ in MR.get_many(layers[3:], probes[:500])]


def test_golden_store_scan_before_the_flush(store):
    """scan_ranges(level 0, ranges, memtables=...) equals the reference store's scan after close()
    flushed its memtables."""
    layers, mts, tables = store
    ranges = [(g["lower"], g["upper"]) for g in STORE["scans"]]
    pr, ro = scan_ranges(tables[:3], ranges, memtables=mts)
    got = records_of(pr)
    assert len(ro) == len(ranges) + 1 and ro[0] == 0 and int(ro[-1]) == pr.n
    for q, g in enumerate(STORE["scans"]):
        part = got[int(ro[q]):int(ro[q + 1])]
        assert len(part) == g["records"], g["name"]
        assert (sha(k for k, _ in part), sha(v for _, v in part)) == (g["keys_sha256"], g["values_sha256"]), g["name"]
    assert count_ranges(tables[:3], ranges, memtables=mts).tolist() == [g["windows"] for g in STORE["scans"]]
    one = scan_tables(tables[:3], ranges[0][0], ranges[0][1], memtables=mts)
    assert records_of(one) == got[int(ro[0]):int(ro[1])]
    # the device-pointer form gives the same run
    assert scan_device(mts, tables[:3], ranges) == (got, ro.tolist())


def scan_device(mts, tables, ranges, stream=None):
    """pbf_mt_scan with device outputs on torch's current (or the given) stream."""
    b = _Bounds(ranges)
    hs = _handles(tables) if tables else None
    n, kb, vb, _, _ = _size(hs, len(tables), b, False, _mt_handles(mts), len(mts))
    dev = torch.device("cuda", mts[0].device)
    keys = torch.full((kb + 64,), GUARD, dtype=torch.uint8, device=dev)
    vals = torch.full((vb + 64,), GUARD, dtype=torch.uint8, device=dev)
    ko = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    vo = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    ro = torch.zeros(b.n + 1, dtype=torch.int64, device=dev)
    tot = [ctypes.c_uint64() for _ in range(3)]
    s = stream or torch.cuda.current_stream(dev)
    rc = _native.lib().pbf_mt_scan(_mt_handles(mts), len(mts), hs, len(tables), *b.args(), vp(keys.data_ptr()), kb,
                                   vp(ko.data_ptr()), vp(vals.data_ptr()), vb, vp(vo.data_ptr()), n + 1,
                                   *[ctypes.byref(t) for t in tot], vp(ro.data_ptr()), 1, vp(s.cuda_stream or None))
    _native.check(rc, "pbf_mt_scan")
    s.synchronize()
    m, mk, mv = (t.value for t in tot)
    assert (keys[mk:] == GUARD).all() and (vals[mv:] == GUARD).all()
    pr = PackedRecords(PackedKeys(keys[:mk].cpu().numpy(), m, offsets=ko[:m + 1].cpu().numpy().view(np.uint64)),
                       vals[:mv].cpu().numpy(), vo[:m + 1].cpu().numpy().view(np.uint64))
    return records_of(pr), ro.cpu().tolist()


# ------------------------------------------------------------------ apply
@pytest.mark.parametrize("n", [1, T - 1, T, T + 1])
def test_apply_batch_sizes_at_the_sort_tile(n, made):
    order = np.random.default_rng(n).permutation(n).tolist()
    first = [(f"{j:06d}", value(p)) for p, j in enumerate(order)]
    m = made.mt(first)
    assert records_of(m.records()) == run_of(first) == records_of(sort_log(first))
    second = [(f"{(j * 3) % (n + 5):06d}", value(p + 7)) for p, j in enumerate(order)]
    m.put_many(second)
    assert records_of(m.records()) == run_of(first + second) and len(m) == len(run_of(first + second))


def test_apply_batch_that_only_repeats_one_key(made):
    m = made.mt([("k5", value(i)) for i in range(T + 3)])
    assert records_of(m.records()) == [(b"k5", value(T + 2))]
    m.put_many([("k5", b"")] * 3)
    assert records_of(m.records()) == [(b"k5", b"")] and m.get("k5") == b""
    m.put_many([("k4", b"x"), ("k6", b"y")])
    assert records_of(m.records()) == [(b"k4", b"x"), (b"k5", b""), (b"k6", b"y")]


@pytest.mark.parametrize("second", ["below", "above", "interleaved", "equal", "superset"])
def test_apply_second_batch_against_the_resident_run(second, made):
    base = [(f"m{i:05d}", value(i)) for i in range(0, 3000, 2)]
    batch = {"below": [(f"a{i:05d}", value(i + 1)) for i in range(700)],
             "above": [(f"z{i:05d}", value(i + 2)) for i in range(700)],
             "interleaved": [(f"m{i:05d}", value(i + 3)) for i in range(1, 3000, 2)],
             "equal": [(k, value(i + 4, 3)) for i, (k, _) in enumerate(reversed(base))],
             "superset": [(f"m{i:05d}", value(i + 5, i % 4)) for i in range(3000)]}[second]
    m = made.mt(base, batch)
    want = run_of(base + batch)
    assert records_of(m.records()) == want
    if second == "equal":  # the new batch wins every shared key
        assert all(len(v) == 3 for _, v in want) and len(want) == len(base)
    probes = [k for k, _ in base[::7]] + [k for k, _ in batch[::5]] + ["m", "zz", ""]
    assert m.get_many(probes) == [MR.ModelMemTable(base + batch).get(k) for k in probes]


def test_ten_successive_applies_equal_the_concatenated_log(made):
    m, log = made.mt(), []
    for r in range(10):
        n = [1, 5, 300, T + 1, 2, 700, 1, 3 * T, 40, 9][r]
        batch = [(f"k{MT.mix(r, i) % 4000:05d}", value(r * 10000 + i)) for i in range(n)]
        log += batch
        m.put_many(batch)
        assert records_of(m.records()) == run_of(log) == records_of(sort_log(log))
    assert m.approximate_size == sum(8 + len(k) + len(v) for k, v in log)


def test_single_puts_are_buffered_and_applied_by_the_next_read(made):
    m = made.mt()
    assert m.get("a") is None and len(m) == 0 and records_of(m.records()) == [] and records_of(m.scan("", "")) == []
    with pytest.raises(ValueError, match="at least one record"):
        m.flush_resident()
    m.put("b", b"1")
    m.put("a", b"")
    m.put("b", b"22")
    assert (m.get("b"), m.get("a"), m.get("c")) == (b"22", b"", None)
    m.put("c", b"3")
    m.sync()
    assert records_of(m.records()) == [(b"a", b""), (b"b", b"22"), (b"c", b"3")] and len(m) == 3
    assert m.approximate_size == 10 + 9 + 11 + 10


# ------------------------------------------------------------------ search
def windows_of(m, bounds):
    """[lo, hi) per (lower, upper) over one memtable, from pbf_mt_scan_size."""
    b = _Bounds(bounds)
    _, _, _, lo, hi = _size(None, 0, b, True, _mt_handles([m]), 1)
    return list(zip(lo[:, 0].tolist(), hi[:, 0].tolist()))


@pytest.mark.parametrize("alphabet,prefix", [("\0a", ""), ("ab", "prefix00"), ("\0a", "12345678")])
def test_search_prefix_ties_at_every_step(alphabet, prefix, made):
    """All strings of 0..10 characters over a two-letter alphabet (behind a shared 8-byte prefix:
    every step of the search is a prefix tie): two thirds stored, all probed, for equality and for
    the lower bound."""
    strings = [prefix + "".join(t) for n in range(11) for t in itertools.product(alphabet, repeat=n)]
    stored = [s for i, s in enumerate(strings) if i % 3]
    rows = [(s, value(i)) for i, s in enumerate(stored)]
    m = made.mt(rows)
    keys = sorted(s.encode() for s in stored)
    assert [k for k, _ in records_of(m.records())] == keys
    check_get([m], [run_of(rows)], strings)
    wins = windows_of(m, [(s, s) for s in strings] + [(s, "") for s in strings[::5]])
    for s, (lo, hi) in zip(strings + strings[::5], wins):
        lb, eq = MR.lower_bound(keys, s)
        assert lo == lb
    for s, (lo, hi) in zip(strings, wins):  # upper == lower ("" as upper is open)
        assert hi == (lo + int(s.encode() in set(keys[lo:lo + 1])) if s else len(keys))
    assert [hi for _, hi in wins[len(strings):]] == [len(keys)] * len(strings[::5])


def test_search_key_lengths_around_the_prefix_and_high_probe_bytes(made):
    base = "abcdefghijklmnopqrstuvwxyz"
    stored = sorted({base[:n] for n in (7, 8, 9, 16, 17)} | {base[:7] + "z", base[:8] + "\0", base[:16] + "\0"})
    rows = [(s, value(i)) for i, s in enumerate(stored)]
    m = made.mt(rows)
    probes = [s.encode() for s in stored] + [base[:n].encode() for n in range(0, 20)]
    for s in stored:  # bytes >= 0x80 at bytes 0, 7 and 8, against ASCII stored keys
        for at in (0, 7, 8):
            for byte in (0x80, 0xC3, 0xFF):
                if at < len(s):
                    probes.append(s.encode()[:at] + bytes([byte]) + s.encode()[at + 1:])
                probes.append(s.encode()[:at] + bytes([byte]))
    want = check_get([m], [run_of(rows)], raw_keys(probes))
    assert sum(v is not None for v, _ in want) == len(stored) + 5
    wins = windows_of(m, [("é", ""), (base[:7] + "é", ""), (base[:8] + "€", base[:8] + "€")])
    keys = [s.encode() for s in stored]
    assert wins == [(len(keys), len(keys)), (bisect_left(keys, (base[:7] + "é").encode()), len(keys)),
                    (bisect_left(keys, (base[:8] + "€").encode()),) * 2]


def test_search_one_record_and_probes_outside(made):
    m = made.mt([("middle", b"v")])
    check_get([m], [[("middle", b"v")]], ["", "a", "middl", "middle", "middle\0", "middlf", "z", "\x7f"])
    assert windows_of(m, [("", ""), ("a", "b"), ("n", ""), ("middle", "middle"), ("z", "a")]) == \
        [(0, 1), (0, 0), (1, 1), (0, 1), (1, 1)]
    big = made.mt([(f"k{i:04d}", value(i)) for i in range(100, 900)])
    check_get([big], [[(f"k{i:04d}", value(i)) for i in range(100, 900)]], ["k0099", "k0100", "k0899", "k0900", "j", "l"])


# ------------------------------------------------------------------ get stage
def raw_get(mts, pk, on_device=False):
    """pbf_mt_get with 64 guard bytes around every output: (src, val_off, val_len, mask)."""
    n, nb = pk.n, (pk.n + 7) // 8
    L = _native.lib()
    hs = _mt_handles(mts)
    if not on_device:
        bufs = [np.full(64 + n * w + 64, GUARD, dtype=np.uint8) for w in (4, 8, 4)] + [np.full(64 + nb + 64, GUARD, np.uint8)]
        kd = pk.data if pk.data.size else np.zeros(1, np.uint8)
        rc = L.pbf_mt_get(hs, len(mts), vp(kd.ctypes.data), None if pk.offsets is None else vp(pk.offsets.ctypes.data),
                          pk.key_len, n, 0, None, *[vp(b.ctypes.data + 64) for b in bufs])
        _native.check(rc, "pbf_mt_get")
    else:
        dev = torch.device("cuda", mts[0].device)
        dbufs = [torch.full((64 + n * w + 64,), GUARD, dtype=torch.uint8, device=dev) for w in (4, 8, 4)] + \
                [torch.full((64 + nb + 64,), GUARD, dtype=torch.uint8, device=dev)]
        o0 = int(pk.offsets[0]) if pk.offsets is not None else 0
        kd = torch.from_numpy(np.ascontiguousarray(pk.data[o0:]) if pk.data.size > o0 else np.zeros(1, np.uint8)).to(dev)
        od = None if pk.offsets is None else torch.from_numpy(pk.offsets.view(np.int64).copy()).to(dev)
        s = torch.cuda.current_stream(dev)
        rc = L.pbf_mt_get(hs, len(mts), vp(kd.data_ptr()), None if od is None else vp(od.data_ptr()), pk.key_len, n, 1,
                          vp(s.cuda_stream or None), *[vp(b.data_ptr() + 64) for b in dbufs])
        _native.check(rc, "pbf_mt_get")
        s.synchronize()
        bufs = [b.cpu().numpy() for b in dbufs]
    for b in bufs:
        assert (b[:64] == GUARD).all() and (b[-64:] == GUARD).all()
    return (bufs[0][64:-64].view(np.int32), bufs[1][64:-64].view(np.uint64), bufs[2][64:-64].view(np.int32),
            bufs[3][64:-64])


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
def test_get_every_mask_tail_with_guards(on_device, made):
    """n = 1..257 keys: every tail of the miss mask's last word and byte, pad bits zero, nothing
    written outside the outputs."""
    rows = [(f"k{i:04d}", value(i)) for i in range(0, 600, 2)]
    m = made.mt(rows)
    model = MR.ModelMemTable(rows)
    for n in range(1, 258):
        probes = [f"k{(i * 7 + n) % 600:04d}" for i in range(n)]
        if n % 3 == 0:
            probes = [p + "x" * (i % 3) for i, p in enumerate(probes)]  # variable length
        want = [model.get(p) for p in probes]
        src, vo, vl, mask = raw_get([m], PackedKeys.from_strs(probes), on_device)
        assert src.tolist() == [-1 if v is None else 0 for v in want], n
        assert vl.tolist() == [-1 if v is None else len(v) for v in want], n
        bits = np.unpackbits(mask, bitorder="little")
        assert bits[:n].tolist() == [int(v is None) for v in want] and not bits[n:].any(), n


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
def test_get_a_window_of_a_key_batch(on_device, made):
    rows = [(f"key{i:03d}", value(i)) for i in range(50)]
    m = made.mt(rows)
    keys = [b"zz", b"key001", b"key01", b"key049", b"", b"key0500", b"key007"]
    whole = raw_keys(keys)
    win = PackedKeys(whole.data, 4, offsets=whole.offsets[2:7].copy())  # keys[2:6]: offsets[0] != 0
    src, vo, vl, mask = raw_get([m], win, on_device)
    assert src.tolist() == [-1, 0, -1, -1] and vl.tolist() == [-1, len(value(49)), -1, -1] and mask.tolist() == [0b1101]


def test_get_sixteen_memtables_and_the_first_holder_answers(made):
    mts, layers = [], []
    for u in range(16):
        rows = [(f"own{u:02d}", value(u, 4))]
        if u in (3, 9):
            rows.append(("shared", value(u, 5)))
        if u in (5, 11):
            rows.append(("emptyfirst", b"" if u == 5 else b"older"))
        rows.sort()
        mts.append(made.mt(rows))
        layers.append(rows)
    probes = ["shared", "emptyfirst", "absent"] + [f"own{u:02d}" for u in range(16)]
    want = check_get(mts, layers, probes)
    assert [u for _, u in want][:3] == [3, 5, -1] and want[1][0] == b""
    with pytest.raises(ValueError, match="at most 16 memtables, got 17"):
        mt_lookup(mts + [made.mt([("x", b"y")])], probes)
    hs17 = (vp * 17)(*([m._handle().value for m in mts] + [mts[0]._handle().value]))
    out = np.zeros(8, dtype=np.uint64)
    key = np.frombuffer(b"shared", dtype=np.uint8)
    rc = _native.lib().pbf_mt_get(hs17, 17, vp(key.ctypes.data), None, 6, 1, 0, None, vp(out.ctypes.data),
                                  vp(out.ctypes.data), vp(out.ctypes.data), vp(out.ctypes.data))
    assert rc == _native.PBF_ERR_INVALID and b"at most 16 memtables, got 17" in _native.lib().pbf_last_error()
    rc = _native.lib().pbf_mt_get(hs17, 2, vp(key.ctypes.data), None, 6, 1, 0, None, vp(out.ctypes.data),
                                  vp(out.ctypes.data), vp(out.ctypes.data), vp(out.ctypes.data))
    assert rc == _native.PBF_OK
    hs_twice = (vp * 2)(mts[0]._handle().value, mts[0]._handle().value)
    rc = _native.lib().pbf_mt_get(hs_twice, 2, vp(key.ctypes.data), None, 6, 1, 0, None, vp(out.ctypes.data),
                                  vp(out.ctypes.data), vp(out.ctypes.data), vp(out.ctypes.data))
    assert rc == _native.PBF_ERR_INVALID and b"listed twice" in _native.lib().pbf_last_error()


def test_get_batch_numbering_and_empty_values_across_memtables_and_tables(made):
    """table[i] = -2 - m for memtable m, the table's row otherwise, -1 for none; an empty value in
    the newest holder wins over an older non-empty one, in a memtable and in a table behind it; a
    key a memtable answered is searched in no table."""
    m0 = made.mt([("a", b""), ("b", b"m0"), ("f", b"m0f")])
    m1 = made.mt([("a", b"old"), ("c", b""), ("d", b"m1")])
    t0 = made.table([("c", b"t0c"), ("e", b""), ("g", b"t0")])
    t1 = made.table([("e", b"t1e"), ("f", b"t1f"), ("h", b"t1")])
    keys = list("abcdefghi") + [""]
    layers = [[("a", b""), ("b", b"m0"), ("f", b"m0f")], [("a", b"old"), ("c", b""), ("d", b"m1")],
              [("c", b"t0c"), ("e", b""), ("g", b"t0")], [("e", b"t1e"), ("f", b"t1f"), ("h", b"t1")]]
    want = MR.get_many(layers, keys)
    for level0, levels in (([t0, t1], []), ([t0], [[t1]])):
        table, vals, offs = lsm_get.get_batch(keys, level0, levels, memtables=[m0, m1])
        assert table.tolist() == [-2, -2, -3, -3, 0, -2, 0, 1, -1, -1]
        raw = vals.tobytes()
        assert [raw[int(offs[i]):int(offs[i + 1])] if table[i] != -1 else None for i in range(len(keys))] == [v for v, _ in want]
        assert lsm_get.get_many(keys, level0, levels, memtables=[m0, m1]) == [v for v, _ in want]
    assert lsm_get.get_many(keys, [t0, t1], [], memtables=[m1, m0])[0] == b"old"
    timings = {}
    kd = torch.from_numpy(np.frombuffer(b"abcdefghi", dtype=np.uint8).copy()).cuda()
    table, _, _, _ = lsm_get._walk_device(kd.data_ptr(), 0, 1, 9, [t0, t1], [], m0.device, timings, memtables=[m0, m1])
    assert table.tolist() == [-2, -2, -3, -3, 0, -2, 0, 1, -1] and "memtable_ms" in timings


# ------------------------------------------------------------------ gather
def test_gather_every_source_and_destination_alignment(made):
    """Every (source offset mod 16, destination offset mod 16, length 0..40) for memtable values,
    with the output base at +0 and +5, memtable and table hits mixed in one batch."""
    rows, off = [], 0
    for j in range(16):
        rows.append((f"a-pad{j:02d}", bytes([0x40 + j]) * j))
        off += j
    targets = []
    for s in range(16):
        for L in range(41):
            pad = (s - off) % 16
            rows.append((f"b{len(targets):04d}-pad", bytes([0x30 + s]) * pad))
            off += pad
            assert off % 16 == s
            rows.append((f"b{len(targets):04d}-val", MT.value_of(s * 41 + L, L)))
            off += L
            targets.append((f"b{len(targets):04d}-val", s, L))
    m = made.mt(rows)
    trows = [(f"t{i:03d}", MT.value_of(1000 + i, i % 41)) for i in range(200)]
    t = made.table(trows)
    probes, dest = [], 0
    for d in range(16):
        for i, (key, s, L) in enumerate(targets):
            pad = (d - dest) % 16
            probes.append(f"a-pad{pad:02d}")
            dest += pad
            probes.append(key)
            dest += L
            if i % 9 == 0:
                probes.append(trows[(i + d) % 200][0])
                dest += len(trows[(i + d) % 200][1])
    want = MR.get_many([rows, trows], probes)
    src, vo, vl, _ = mt_lookup([m], probes)
    assert {(int(o) % 16, l) for o, l, u in zip(vo, vl, src) if u == 0 and l > 0} >= {(s, L) for s in range(16) for L in range(1, 41)}
    ttab, tvo, tvl = lookup([t], probes)
    where = np.where(src >= 0, -2 - src, ttab).astype(np.int32)
    val_off = np.where(src >= 0, vo, tvo)
    val_len = np.where(src >= 0, vl, tvl).astype(np.int32)
    assert where.tolist() == [-2 if u == 0 else (0 if u == 1 else -1) for _, u in want]
    expect = b"".join(v for v, _ in want if v)
    vals, offs = mt_gather([m], [t], where, val_off, val_len)  # host pointers
    assert vals.tobytes() == expect and offs.tolist() == list(np.cumsum([0] + [len(v or b"") for v, _ in want]))
    assert {(int(o) % 16) for o in offs[:-1]} == set(range(16))
    dev = torch.device("cuda", m.device)
    dw, dvo, dvl = (torch.from_numpy(a.copy()).to(dev) for a in (where, val_off.view(np.int64), val_len))
    for base in (0, 5):  # device pointers: the output starts at any byte
        out = torch.full((64 + base + len(expect) + 64,), GUARD, dtype=torch.uint8, device=dev)
        doffs = torch.zeros(len(probes) + 1, dtype=torch.int64, device=dev)
        s = torch.cuda.current_stream(dev)
        rc = _native.lib().pbf_mt_gather(_mt_handles([m]), 1, _handles([t]), 1, vp(dw.data_ptr()), vp(dvo.data_ptr()),
                                         vp(dvl.data_ptr()), len(probes), vp(out.data_ptr() + 64 + base), len(expect),
                                         vp(doffs.data_ptr()), 1, vp(s.cuda_stream or None))
        _native.check(rc, "pbf_mt_gather")
        s.synchronize()
        o = out.cpu().numpy()
        assert o[64 + base:64 + base + len(expect)].tobytes() == expect
        assert (o[:64 + base] == GUARD).all() and (o[64 + base + len(expect):] == GUARD).all()
        assert doffs.cpu().tolist() == offs.tolist()
    # an entry that names no source, or lies outside its source's bytes, is refused
    at = next(i for i in range(len(probes)) if src[i] == 0 and vl[i] > 1)
    bad = where.copy()
    bad[at] = -3
    with pytest.raises(ValueError, match="name no source or lie outside"):
        mt_gather([m], [t], bad, val_off, val_len)
    far = val_off.copy()
    far[at] = off - 1
    with pytest.raises(ValueError, match="name no source or lie outside"):
        mt_gather([m], [t], where, far, val_len)


# ------------------------------------------------------------------ scan
def model_runs(layers, ranges):
    return [[(k, v) for k, v, _ in MR.scan(layers, lo, up)] for lo, up in ranges]


def check_scan(mts, tables, layers, ranges):
    pr, ro = scan_ranges(tables, ranges, memtables=mts)
    got = records_of(pr)
    assert len(ro) == len(ranges) + 1 and ro[0] == 0 and int(ro[-1]) == pr.n
    for q, w in enumerate(model_runs(layers, ranges)):
        assert got[int(ro[q]):int(ro[q + 1])] == w, (q, ranges[q])
    want_counts = [[hi - lo for lo, hi in MR.windows(layers, lo_, up_)] for lo_, up_ in ranges]
    assert count_ranges(tables, ranges, memtables=mts).tolist() == want_counts
    return got, ro


@pytest.mark.parametrize("case", SM.CASES, ids=[c["name"] for c in SM.CASES])
def test_scan_every_range_rule_over_mixed_sources(case, made):
    """lsm_scan.json's range rules over 1 memtable + 0 tables, 3 memtables + 3 tables, and a memtable
    that holds every key in front of the tables (fully shadowed); the first against the golden
    hashes of the one-table scan too."""
    rows = MM.case_tables(case)
    gold = next(c for c in SCAN_CASES if c["name"] == case["name"])
    ranges = [(lo, up) for _, lo, up in SM.case_ranges(case)]
    assert ranges == [(g["lower"], g["upper"]) for g in gold["ranges"]]
    # 1 memtable + 0 tables
    m = made.mt(rows[0])
    got, ro = check_scan([m], [], [rows[0]], ranges)
    assert [int(ro[q + 1] - ro[q]) for q in range(len(ranges))] == [g["table_records"][0] for g in gold["ranges"]]
    assert records_of(m.scan(*ranges[0])) == got[int(ro[0]):int(ro[1])]
    # the case's tables as memtables (up to 3) in front of three more tables
    other = MM.case_tables(next(c for c in MM.CASES if c["name"] == "shadowed"))
    layers = rows[:3] + other
    mts = [made.mt(r) for r in rows[:3]]
    tables = [made.table(r) for r in other]
    got, ro = check_scan(mts, tables, layers, ranges)
    if len(rows) == 3:  # the golden run of the case is the memtables' part where no other table is hit
        for q, g in enumerate(gold["ranges"]):
            if all(hi == lo for lo, hi in MR.windows(other, *ranges[q])):
                part = got[int(ro[q]):int(ro[q + 1])]
                assert (len(part), sha(k for k, _ in part)) == (g["records"], g["keys_sha256"])
    # a memtable that holds every key: the tables are fully shadowed
    union = sorted({k for r in layers for k, _ in r})
    cover = [(k, value(i, i % 3)) for i, k in enumerate(union)]
    mc = made.mt(cover)
    got, _ = check_scan([mc], tables, [cover] + other, ranges)
    assert all(v == dict(cover)[k.decode()] for k, v in got)


@pytest.mark.parametrize("n", [T, T + 1])
def test_scan_selected_records_at_the_scan_tile(n, made):
    a = [(f"k{i:06d}", value(i)) for i in range(0, n, 2)]
    b = [(f"k{i:06d}", value(i + 1)) for i in range(1, n, 2)]
    c = [(f"k{i:06d}", value(i + 2)) for i in range(0, n, 64)]
    ma, mb, tc = made.mt(a), made.mt(b), made.table(c)
    got, _ = check_scan([ma, mb], [tc], [a, b, c], [("", ""), ("k000001", f"k{n - 2:06d}"), ("k0", "k0")])
    assert len(got) == n + (n - 2)


def test_scan_past_the_scans_carry(made):
    """524,289 selected records: 257 scan tiles, the tile scan's second chunk."""
    n = 256 * T + 1
    keys = np.char.add("k", np.char.zfill(np.arange(n).astype(str), 7)).tolist()
    half = [(k, b"m" if i % 3 else b"") for i, k in enumerate(keys) if i % 2 == 0]
    rest = [(k, b"tt") for i, k in enumerate(keys) if i % 2]
    shadow = [(keys[i], b"old") for i in range(0, n, 1000)]
    m, m2, t = made.mt(half), made.mt(rest), made.table(shadow, 4096)
    pr, ro = scan_ranges([t], [("", ""), (keys[5], keys[5])], memtables=[m, m2])
    assert ro.tolist() == [0, n, n + 1] and pr.n == n + 1
    assert pr.keys.data.tobytes() == "".join(keys).encode() + keys[5].encode()
    want_vals = b"".join((b"m" if i % 3 else b"") if i % 2 == 0 else b"tt" for i in range(n)) + b"tt"
    assert np.asarray(pr.values).tobytes() == want_vals
    assert count_ranges([t], [("", "")], memtables=[m, m2]).tolist() == [[len(half), len(rest), len(shadow)]]


def test_scan_capacities_one_short_write_nothing(made):
    a = [(f"k{i:04d}", value(i)) for i in range(300)]
    b = [(f"k{i:04d}", value(i + 9)) for i in range(150, 450)]
    m, t = made.mt(a), made.table(b)
    ranges = [("k0100", "k0399"), ("", "k0005")]
    bounds = _Bounds(ranges)
    want = [r for run in model_runs([a, b], ranges) for r in run]
    n, kb, vb = len(want), sum(len(k) for k, _ in want), sum(len(v) for _, v in want)
    L = _native.lib()
    for short in ("keys", "values", "offsets", None):
        caps = {"keys": kb, "values": vb, "offsets": n + 1}
        if short:
            caps[short] -= 1
        keys = np.full(64 + kb + 64, GUARD, np.uint8)
        vals = np.full(64 + vb + 64, GUARD, np.uint8)
        ko, vo = np.full(n + 9, 0x5A5A, np.uint64), np.full(n + 9, 0x5A5A, np.uint64)
        ro = np.full(len(ranges) + 9, 0x5A5A, np.uint64)
        tot = [ctypes.c_uint64() for _ in range(3)]
        rc = L.pbf_mt_scan(_mt_handles([m]), 1, _handles([t]), 1, *bounds.args(), vp(keys.ctypes.data + 64), caps["keys"],
                           vp(ko.ctypes.data), vp(vals.ctypes.data + 64), caps["values"], vp(vo.ctypes.data),
                           caps["offsets"], *[ctypes.byref(x) for x in tot], vp(ro.ctypes.data), 0, None)
        assert [x.value for x in tot] == [n, kb, vb]
        if short:
            assert rc == _native.PBF_ERR_INVALID
            need = {"keys": f"the keys need {kb} bytes, keys_out holds {kb - 1}",
                    "values": f"the values need {vb} bytes, values_out holds {vb - 1}",
                    "offsets": f"needs {n + 1} entries, offsets_cap is {n}"}[short]
            assert need in L.pbf_last_error().decode()
            assert (keys == GUARD).all() and (vals == GUARD).all()
            assert (ko == 0x5A5A).all() and (vo == 0x5A5A).all() and (ro == 0x5A5A).all()
        else:
            assert rc == _native.PBF_OK
            assert keys[64:64 + kb].tobytes() == b"".join(k for k, _ in want) and (keys[64 + kb:] == GUARD).all()
            assert vals[64:64 + vb].tobytes() == b"".join(v for _, v in want) and (vals[:64] == GUARD).all()
            assert (ko[n + 1:] == 0x5A5A).all() and (ro[len(ranges) + 1:] == 0x5A5A).all() and ro[len(ranges)] == n


def test_scan_empty_memtable_among_others_and_refusals(made):
    a = [(f"k{i:03d}", value(i)) for i in range(0, 100, 2)]
    b = [(f"k{i:03d}", value(i + 1)) for i in range(0, 100, 3)]
    ma, me, mb = made.mt(a), made.mt(), made.mt(b)
    ranges = [("", ""), ("k010", "k050"), ("k051", "k050"), ("zz", "")]
    check_scan([ma, me, mb], [], [a, [], b], ranges)
    check_scan([me], [], [[]], ranges)
    t = made.table(b)
    check_scan([me, ma], [t], [[], a, b], ranges)
    assert records_of(scan_ranges([t], [], memtables=[ma])[0]) == []
    with pytest.raises(ValueError, match="listed twice"):
        scan_ranges([], ranges, memtables=[ma, ma])
    with pytest.raises(ValueError, match="at most 64 memtables and tables together"):
        scan_ranges([t] * 63, ranges, memtables=[ma, mb])
    with pytest.raises(ValueError, match="ranges x sources"):
        scan_ranges([t], [("a", "b")] * (2 ** 21 + 1), memtables=[ma])
    L = _native.lib()
    z = ctypes.c_uint64()
    rc = L.pbf_mt_scan_size(None, 0, _handles([t]), 1, *_Bounds(ranges).args(), None, None, ctypes.byref(z),
                            ctypes.byref(z), ctypes.byref(z))
    assert rc == _native.PBF_ERR_INVALID and b"no memtables" in L.pbf_last_error()


# ------------------------------------------------------------------ flush
def test_flush_resident_spanning_several_blocks(made):
    puts = [(f"key-{MT.mix(9, i) % 5000:05d}", value(i, 20 + i % 60)) for i in range(6000)]
    m = made.mt(puts[:2500], puts[2500:])
    want, metas, _ = flush_log(puts, block_size=4096)
    assert len(metas) > 20
    table = m.flush_resident(block_size=4096)
    try:
        assert table.to_bytes().tobytes() == want.tobytes()
        assert table.nrecords == len(m) and (table.first_key, table.last_key) == (metas[0][0], metas[-1][1])
        # the flushed table behind the memtable it came from answers as the memtable does
        probes = [k for k, _ in puts[::37]] + ["key-", "zzz"]
        assert lsm_get.get_many(probes, [table], []) == m.get_many(probes)
    finally:
        table.close()
    with pytest.raises(ValueError, match="larger than block_size"):
        m.flush_resident(block_size=64)


# ------------------------------------------------------------------ lifetime
def test_closed_and_destroyed_handles_are_refused(made):
    m = DeviceMemTable()
    m.put_many([("a", b"1")])
    h = m._handle().value
    L = _native.lib()
    z = ctypes.c_uint64()
    assert L.pbf_mt_info(vp(h), ctypes.byref(z), None, None) == _native.PBF_OK and z.value == 1
    m.close()
    for call in (lambda: m.get("a"), lambda: m.put("b", b"2"), lambda: m.put_many([("b", b"2")]), lambda: m.records(),
                 lambda: m.scan("", ""), lambda: m.flush_resident(), lambda: len(m), lambda: m.sync()):
        with pytest.raises(ValueError, match="the memtable is closed"):
            call()
    # the destroyed handle is refused by pointer value, by every entry
    assert L.pbf_mt_info(vp(h), ctypes.byref(z), None, None) == _native.PBF_ERR_INVALID
    assert L.pbf_mt_apply(vp(h), None, None, None, None, 0) == _native.PBF_ERR_INVALID
    assert L.pbf_mt_destroy(vp(h)) == _native.PBF_ERR_INVALID
    job = vp()
    assert L.pbf_mt_flush_begin(vp(h), 4096, ctypes.byref(job)) == _native.PBF_ERR_INVALID and not job.value
    assert L.pbf_mt_destroy(None) == _native.PBF_OK


def test_get_on_a_side_stream_then_apply_after_reads(made):
    """A get queued on a non-default stream between the upload of its keys and the reader of its
    results; the apply that follows waits for it before it frees the run it read."""
    rows = [(f"k{i:05d}", value(i)) for i in range(5000)]
    m = made.mt(rows)
    dev = torch.device("cuda", m.device)
    probes = [f"k{(i * 13) % 6000:05d}" for i in range(4096)]
    pk = PackedKeys.from_strs(probes)
    side = torch.cuda.Stream(dev)
    host = torch.from_numpy(pk.data.copy()).pin_memory()
    with torch.cuda.stream(side):
        kd = host.to(dev, non_blocking=True)
        src = torch.empty(pk.n, dtype=torch.int32, device=dev)
        vo = torch.empty(pk.n, dtype=torch.int64, device=dev)
        vl = torch.empty(pk.n, dtype=torch.int32, device=dev)
        mask = torch.empty((pk.n + 7) // 8, dtype=torch.uint8, device=dev)
        rc = _native.lib().pbf_mt_get(_mt_handles([m]), 1, vp(kd.data_ptr()), None, pk.key_len, pk.n, 1,
                                      vp(side.cuda_stream), vp(src.data_ptr()), vp(vo.data_ptr()), vp(vl.data_ptr()),
                                      vp(mask.data_ptr()))
        _native.check(rc, "pbf_mt_get")
        hits = (src >= 0).sum()
    m.put_many([(f"k{i:05d}", b"new") for i in range(4000, 6000)])  # apply after the read: waits for its event
    side.synchronize()
    model = dict(rows)
    assert int(hits) == sum(p in model for p in probes)
    assert vl.cpu().tolist() == [len(model[p]) if p in model else -1 for p in probes]
    assert m.get_many(["k04000", "k05999", "k03999"]) == [b"new", b"new", value(3999)]
    assert len(m) == 6000
